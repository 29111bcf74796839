"""Sphere-list kernel (kind 16): camera rays tested against their tile's candidate list (primary rounds of render_kernel,
csrc/primary_cull_rule.h) against the scan of the whole list.

A list holds every sphere the reference could accept for a camera ray of its tile, in list order, and the listed spheres go through
the reference's own test: frames do not change.  For every case and both builds the default launch equals
RT_FLAG_NO_PRIMARY_LISTS, RT_FLAG_EXACT_SCAN and RT_FLAG_FILTER_FP64 in the frame, in the frame continued from the saved RNG
streams and in both ray counts; the strict build also equals the CPU oracle bit for bit.  64 x 48, 4 samples plus 2 continued,
depth 8, unless the case says otherwise.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import primary_list_worlds as P
from conftest import build_both
from frame_helpers import render_params
from scan_checks import MORE, SPP, assert_same_scan, assert_strict_equals_oracle, render_twice

pytestmark = pytest.mark.gpu

DEPTH = 8
WORLDS = P.cases()

# name -> (world, keywords): width / height, depth, film (Film keywords), render (render keywords), flags (on every launch),
# adaptive (Film.set_adaptive keywords), sky (every ray is a camera ray that leaves the scene)
CASES = {
    "field_on_ground": ("field_on_ground", {}),
    "sky_only": ("sky_only", dict(sky=True)),
    "camera_inside_glass": ("camera_inside_glass", {}),
    "forty_in_a_row": ("forty_in_a_row", {}),
    "coincident_pair": ("coincident_pair", {}),
    "depth_1": ("field_on_ground", dict(depth=1)),
    "depth_2": ("field_on_ground", dict(depth=2)),
    "61_by_45": ("field_on_ground", dict(width=61, height=45)),
    "rank_1_of_3_stripes_of_8": ("field_on_ground", dict(film=dict(stripe_rows=8, rank=1, world_size=3))),
    "rank_1_of_3_stripes_of_5": ("field_on_ground", dict(film=dict(stripe_rows=5, rank=1, world_size=3))),
    "no_pixel_classes": ("field_on_ground", dict(flags=rt.FLAG_NO_PIXEL_CLASSES)),
    "accumulate": ("field_on_ground", dict(flags=rt.FLAG_ACCUMULATE)),
    "adaptive_film": ("field_on_ground", dict(adaptive=dict(min_samples=2, check_interval=1, noise_threshold=0.2))),
    "8_pixels_per_wave": ("field_on_ground", dict(render=dict(pixels_per_wave=8), ppw=8)),
    "wide_lens": ("lens_radius_two", {}),
    "sphere_contains_lens": ("sphere_contains_lens", {}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_primary_lists_change_nothing(name):
    world_name, kw = CASES[name]
    spheres, build = WORLDS[world_name]
    w, h = kw.get("width", P.W), kw.get("height", P.H)
    if (w, h) != (P.W, P.H):
        build = P.world(spheres, aspect=w / h)
    prod, orc = build_both(build)
    film_kw, depth = kw.get("film", {}), kw.get("depth", DEPTH)
    rows = rt.stripe_rows(h, film_kw.get("stripe_rows", 8), film_kw.get("rank", 0), film_kw.get("world_size", 1))
    want = stats = None
    if "adaptive" not in kw:
        want, stats = orc.render(w, h, SPP, depth=depth, want_stats=True)

    def twice(variant, flags):
        return render_twice(prod, w, h, variant, flags | kw.get("flags", 0), depth=depth, film=film_kw, render=kw.get("render"),
                            adaptive=kw.get("adaptive"))

    for variant in (0, 1):
        got = twice(variant, 0)
        off = twice(variant, rt.FLAG_NO_PRIMARY_LISTS)
        exact = twice(variant, rt.FLAG_EXACT_SCAN)
        fp64 = twice(variant, rt.FLAG_FILTER_FP64)
        for r in (got, off, exact, fp64):
            assert r.kernel_kind & ~512 == 16, "a list of spheres is rendered by the sphere-list kernel (512: its adaptive form)"
            assert r.pixels_per_wave == kw.get("ppw", 64)
        for ref, what in ((off, "no primary lists"), (exact, "exact scan"), (fp64, "fp64 filter")):
            assert_same_scan(got, ref, (name, variant, what))
        if kw.get("sky"):
            # every path is one camera ray into the sky: this is also the check that a wave of fresh lanes alone comes to an end
            assert got.rays == w * h * SPP and got.more_rays == w * h * MORE
        if variant == 0 and want is not None:
            assert_strict_equals_oracle(got, want, stats, rows)


@pytest.mark.parametrize("w, h, spp, rehearses", [(128, 96, 16, False), (256, 256, 64, True)])
def test_rehearsal_with_capped_pixels(w, h, spp, rehearses):
    """The rehearsal (launch_plan.cpp plan_frame) runs the same kernel with a ray cap per pixel: its booked costs, the frame and the
    rays are those of the launch without the lists.  128 x 96 x 16 spp is under the planner's floor for a rehearsal (1024 tiles,
    32 samples; 64 for the cap): there the two launches are compared as they are.  256 x 256 x 64 spp is the smallest frame the
    planner rehearses with a cap, and the camera sits in a glass sphere so that some pixels reach it."""
    spheres, _ = WORLDS["camera_inside_glass"]
    prod = P.product(P.world(spheres, aspect=w / h, glass=(len(spheres) - 1,)))
    plan = prod.plan_launch(render_params(w, h, spp))
    assert (plan["probe_spp"] > 0 and plan["pixel_classes"] == 1 and plan["probe_ray_cap"] > 0) == rehearses
    for variant in (0, 1):
        out = []
        for flags in (0, rt.FLAG_NO_PRIMARY_LISTS):
            film = rt.Film(w, h)
            st = film.render(prod, spp, variant=variant, flags=flags, pixels_per_wave=0)
            assert st.kernel_kind == 16 and st.pixels_per_wave == 64
            try:
                costs = film.probe_costs().copy()
            except rt.RtowError as e:
                if "classified no pixels" not in str(e):
                    raise
                costs = None
            out.append((film.download().copy(), st.rays, costs))
        (frame, rays, costs), (frame_off, rays_off, costs_off) = out
        assert (costs is not None) == rehearses and (costs_off is not None) == rehearses
        if rehearses:
            print("pixels the rehearsal stopped at its cap of %d rays: %d" % (plan["probe_ray_cap"], int(np.sum(costs >= plan["probe_ray_cap"]))))
            assert np.any(costs >= plan["probe_ray_cap"]), "no pixel reached the rehearsal's ray cap: the case does not test it"
            assert np.array_equal(costs, costs_off)
        assert rays == rays_off
        assert np.array_equal(frame.view(np.uint64), frame_off.view(np.uint64))
