"""Sphere-list kernel (kind 16): the windows of the pixel-parallel scan's runs (render.hip scan_filtered32,
csrc/scan_window_rule.h) against the scan of every trip.

A pass runs, of a run with a window table, only the trips whose span meets the union of its rays' extents inside the run's slab.
A trip left out holds no sphere the reference could accept (tests/test_scan_windows_host.py), the trips that run do so in list
order, and their survivors go through the reference's test as before: frames do not change.  For every case and both builds the
default launch equals RT_FLAG_NO_SCAN_WINDOWS and RT_FLAG_EXACT_SCAN in the frame, in the frame continued from the saved RNG
streams and in both ray counts; the strict build also equals the CPU oracle bit for bit.  64 x 48 or 67 x 45, 4 samples plus 2
continued, depth 50 unless the case says otherwise.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import primary_list_worlds as P
import scan_segment_lists as S
import scan_window_lists as L
from conftest import Oracle, build_both
from frame_helpers import render_params
from scan_checks import MORE, SPP, assert_same_scan, assert_strict_equals_oracle, render_twice

pytestmark = pytest.mark.gpu

DEPTH = 50
LDS_SPHERE_CAP = 1216  # rows that fit the LDS planes of the sphere-list kernel (tests/test_list_scan_lengths_gpu.py)


def _on_ground():
    """The ground sphere (undecided: its trip always runs), a run on y = 0.3 in ascending x with a glass sphere in it, and a last
    general trip."""
    rnd = np.random.default_rng(2029)
    return [S.GROUND] + L.row(rnd, 63, 1, 0.3, 0, -6.0, 6.0) + S.field(rnd, 8)


def _over_the_cap():
    """1220 rows: two general trips, then a run on y to the padded end, 151 trips in three chunks; rows on the scalar path."""
    rnd = np.random.default_rng(78)
    return S.field(rnd, 16) + L.row(rnd, LDS_SPHERE_CAP + 4 - 16, 1, 0.3, 0, -40.0, 40.0, radius=(0.05, 0.12))


ON_GROUND = _on_ground()
GLASS = 33  # a sphere in the middle of ON_GROUND's run
LISTS = {name: spheres for name, (spheres, _) in L.CASES.items()}
LISTS["on_ground"] = ON_GROUND
LISTS["over_the_lds_cap"] = _over_the_cap()
AXES = {name: axes for name, (_, axes) in L.CASES.items()}
AXES["on_ground"] = [0, None]
AXES["over_the_lds_cap"] = [None, 0]

# name -> (list, keywords): width / height, depth, eye / look, glass, film (Film keywords), render (render keywords), flags (on every
# launch), adaptive (Film.set_adaptive keywords), sky (every ray is a camera ray that leaves the scene)
CASES = {name: (name, {}) for name in LISTS}
CASES.update({
    "67_by_45": ("on_ground", dict(width=67, height=45)),
    "depth_1": ("on_ground", dict(depth=1)),
    "depth_2": ("on_ground", dict(depth=2, width=67, height=45)),
    "above_the_field_sky_only": ("ascending_on_y", dict(eye=(0.0, 6.0, -6.0), look=(4.0, 40.0, -6.0), sky=True)),
    "inside_the_slab_along_it": ("on_ground", dict(eye=(-8.0, 0.3, -6.0), look=(8.0, 0.3, -6.0), width=67, height=45)),
    "inside_a_glass_sphere_of_the_run": ("on_ground", dict(eye=ON_GROUND[GLASS][0], look=(0.0, 0.3, -20.0), glass=(GLASS,))),
    "far_away": ("on_ground", dict(eye=(0.0, 60.0, 250.0), look=(0.0, 0.3, -6.0), vfov=4.0)),
    "rank_1_of_3_stripes_of_5": ("on_ground", dict(film=dict(stripe_rows=5, rank=1, world_size=3))),
    "accumulate": ("on_ground", dict(flags=rt.FLAG_ACCUMULATE)),
    "adaptive_film": ("on_ground", dict(adaptive=dict(min_samples=2, check_interval=1, noise_threshold=0.2))),
    "no_pass_is_pixel_parallel": ("on_ground", dict(render=dict(coop_threshold=65))),
})


def _build(spheres, kw):
    w, h = kw.get("width", L.W), kw.get("height", L.H)
    return P.world(spheres, eye=kw.get("eye", P.EYE), look=kw.get("look", P.LOOK), vfov=kw.get("vfov", 50.0), aspect=w / h, glass=kw.get("glass", ()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_windows_change_nothing(name):
    list_name, kw = CASES[name]
    spheres = LISTS[list_name]
    w, h = kw.get("width", L.W), kw.get("height", L.H)
    prod, orc = build_both(_build(spheres, kw))
    L.check_tables(spheres, prod, AXES[list_name])
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
        off = twice(variant, rt.FLAG_NO_SCAN_WINDOWS)
        exact = twice(variant, rt.FLAG_EXACT_SCAN)
        for r in (got, off, exact):
            assert r.kernel_kind & ~512 == 16, "a list of spheres is rendered by the sphere-list kernel (512: its adaptive form)"
            assert r.pixels_per_wave == 64
        for ref, what in ((off, "no scan windows"), (exact, "exact scan")):
            assert_same_scan(got, ref, (name, variant, what))
        if kw.get("sky"):
            assert got.rays == w * h * SPP and got.more_rays == w * h * MORE
        if variant == 0 and want is not None:
            assert_strict_equals_oracle(got, want, stats, rows)


@pytest.mark.parametrize("w, h", [(64, 48), (67, 45)])
def test_scene_11_itself(w, h):
    """Config C2's list and camera: 60 trips of the run on y = 0.2 with a window on x, the ground's trip and the last general one."""
    prod = rt.builtin_scene(11, 1, w, h)
    wins, _ = prod.scan_windows()
    assert [None if x is None else x[0] for x in wins] == [0, None]
    want = Oracle().render(11, 1, w, h, SPP)
    for variant in (0, 1):
        got = render_twice(prod, w, h, variant, 0)
        off = render_twice(prod, w, h, variant, rt.FLAG_NO_SCAN_WINDOWS)
        exact = render_twice(prod, w, h, variant, rt.FLAG_EXACT_SCAN)
        assert got.kernel_kind == 16 and got.pixels_per_wave == 64
        assert_same_scan(got, off, (variant, "no scan windows"))
        assert_same_scan(got, exact, (variant, "exact scan"))
        if variant == 0:
            assert np.array_equal(got.first.view(np.uint64), want.view(np.uint64))


def test_rehearsal_with_capped_pixels():
    """The rehearsal (launch_plan.cpp plan_frame) runs the same kernel with a ray cap per pixel: its booked costs, the frame and the
    rays are those of the launch without windows.  256 x 256 x 64 spp is the smallest frame the planner rehearses with a cap, and the
    camera sits in a glass sphere of the run so that some pixels reach it."""
    w, h, spp = 256, 256, 64
    prod = P.product(P.world(ON_GROUND, eye=ON_GROUND[GLASS][0], look=(0.0, 0.3, -20.0), aspect=w / h, glass=(GLASS,)))
    plan = prod.plan_launch(render_params(w, h, spp))
    assert plan["probe_spp"] > 0 and plan["pixel_classes"] == 1 and plan["probe_ray_cap"] > 0
    for variant in (0, 1):
        out = []
        for flags in (0, rt.FLAG_NO_SCAN_WINDOWS):
            film = rt.Film(w, h)
            st = film.render(prod, spp, variant=variant, flags=flags, pixels_per_wave=0)
            assert st.kernel_kind == 16 and st.pixels_per_wave == 64
            out.append((film.download().copy(), st.rays, film.probe_costs().copy()))
        (frame, rays, costs), (frame_off, rays_off, costs_off) = out
        assert np.any(costs >= plan["probe_ray_cap"]), "no pixel reached the rehearsal's ray cap: the case does not test it"
        assert np.array_equal(costs, costs_off)
        assert rays == rays_off
        assert np.array_equal(frame.view(np.uint64), frame_off.view(np.uint64))
