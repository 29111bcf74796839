"""Sphere-list kernel (kind 16): the grouped scan's packed fp32 branch, whose survivors are queued and drained per lane
(csrc/render.hip scan_grouped), on windowed lists, against the three scans whose code it leaves alone.

A group of g lanes holds one ray.  A sphere that passes a lane's filter goes to the lane's column of the survivor queue, and the
lanes run the reference's test on their entries in list order behind the last iteration, or sooner where a queue could fill.
Nothing of that may show: for every world, forcing and build the default launch gives the frame, both ray counts and the frame
continued from the saved RNG streams of RT_FLAG_NO_SCAN_WINDOWS, of RT_FLAG_FILTER_FP64 and of RT_FLAG_EXACT_SCAN (tests in place,
as they were), and the strict build equals the CPU oracle bit for bit.  The worlds and cameras were drawn up for a window per
group as well -- a group filtering only the trips its own ray's extent meets (csrc/scan_window_rule.h) -- which was built,
measured and taken out (DESIGN.md section 5 "(r36)"); they stay as the lists on which any skipping of trips by a group would show.

Every pass is sent through the grouped scan (coop_threshold = 65) with 64, 32, ... 1 pixels a wave, i.e. g = 1 ... 64 lanes a ray
as the pixels of a wave end, and on frames 3, 5 and 23 pixels wide that leave groups without a ray.  The worlds:

  * scene 11 as a list (config C2: the ground's trip, 59 more of the run on y = 0.2 with a window on x, the last general trip);
  * the lists of tests/scan_window_lists.py: runs on every axis, in both directions, two windowed runs with a general segment
    between them, a run without a table, more than 64 trips, padding at the end, an undecided row inside a run -- and ON_GROUND,
    with one at the head;
  * a list of 800 rows, above what the packed rows are staged for: the fp64 branch;
  * cameras for each case of the rule: inside the slab looking along it (da = 0 for the middle row of pixels), above the slab
    looking up (every extent empty: only the always-needed trips run), inside a glass sphere that straddles the slab, and 1e6 away
    (the infinite end, the margin at a large |o|);
  * NESTED: 600 concentric spheres inside a windowed run, so that a lane's stride holds more than 16 survivors for every g up to
    32 (at g = 64 a lane's share of 768 rows is 12) and the queue is drained in mid-scan; the outermost radius occurs at seven
    list positions -- neighbours of one pair, of one trip, of different lanes and 16 and more survivors apart -- with a
    different material each, so the first of them in list order must win the tie through the drain and through the reduction;
  * CONCENTRIC: 700 such spheres and nothing else, a list with no window table: the same through the loop over all pairs.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import primary_list_worlds as P
import scan_segment_lists as S
import scan_window_lists as L
from conftest import Oracle, build_both
from scan_checks import Scan, assert_same_scan, assert_strict_equals_oracle

pytestmark = pytest.mark.gpu

SPP, MORE, DEPTH = 8, 4, 50
FORCINGS = [dict(coop_threshold=65)] + [dict(coop_threshold=65, pixels_per_wave=p) for p in (1, 2, 4, 8, 16, 32)]
THIN_FRAMES = [(3, 1), (5, 1), (23, 1)]
REFERENCES = [(rt.FLAG_NO_SCAN_WINDOWS, "no scan windows"), (rt.FLAG_FILTER_FP64, "fp64 filter"), (rt.FLAG_EXACT_SCAN, "exact scan")]


def _on_ground():
    """The ground sphere (undecided: its trip is always needed), a run on y = 0.3 in ascending x, and a last general trip."""
    rnd = np.random.default_rng(2036)
    return [S.GROUND] + L.row(rnd, 63, 1, 0.3, 0, -6.0, 6.0) + S.field(rnd, 8)


def _radius(k, n):
    """Radii between 0.2 and 0.5 in no order along the list; the largest at seven positions."""
    return 0.5 if k in TIES else 0.2 + 0.29 * ((k * 37) % n) / n


TIES = (2, 3, 5, 16, 40, 41, 337)  # one pair; one trip; later trips of other classes; more than a queue of survivors later
NEST_AT = 24                       # the nest begins with trip 3 of the run


def _nested():
    rnd = np.random.default_rng(2037)
    run = L.row(rnd, 64, 1, 0.3, 0, -6.0, 6.0)
    centre = (0.4, 0.3, -5.0)
    nest = [(centre, _radius(k, 600)) for k in range(600)]
    return run[:NEST_AT] + nest + run[NEST_AT:]


def _concentric():
    return [((0.0, 0.3, -5.0), _radius(k, 700)) for k in range(700)]


def _over_the_pairs_cap():
    rnd = np.random.default_rng(2038)
    return S.field(rnd, 16) + L.row(rnd, 784, 1, 0.3, 0, -40.0, 40.0, radius=(0.05, 0.12))


ON_GROUND = _on_ground()
GLASS = 33
LISTS = {name: spheres for name, (spheres, _) in L.CASES.items()}
LISTS.update(on_ground=ON_GROUND, nested=_nested(), concentric=_concentric(), over_the_pairs_cap=_over_the_pairs_cap())
WINDOW_AXES = {name: axes for name, (_, axes) in L.CASES.items()}
WINDOW_AXES.update(on_ground=[0, None], nested=[0], concentric=[None], over_the_pairs_cap=[None, 0])

CASES = {name: (name, {}) for name in LISTS}
CASES.update({
    "inside_the_slab_along_it": ("on_ground", dict(eye=(-8.0, 0.3, -6.0), look=(8.0, 0.3, -6.0), width=63, height=45)),
    "above_the_slab_looking_up": ("on_ground", dict(eye=(0.0, 6.0, -6.0), look=(4.0, 40.0, -6.0), sky=True)),
    "inside_a_glass_sphere_of_the_run": ("on_ground", dict(eye=ON_GROUND[GLASS][0], look=(0.0, 0.3, -20.0), glass=(GLASS,))),
    "a_million_away": ("on_ground", dict(eye=(0.0, 2.4e5, 1.0e6), look=(0.0, 0.3, -6.0), vfov=0.001)),
    "nested_from_behind": ("nested", dict(eye=(0.5, 0.8, -11.0), look=(0.4, 0.3, -5.0))),
    # (a quarter of the frame: 200 nested glass shells make every path long)
    "nested_from_inside": ("nested", dict(eye=(0.4, 0.3, -5.0), look=(0.0, 0.3, -20.0), glass=tuple(NEST_AT + k for k in range(0, 600, 3)),
                                          width=32, height=24)),
})


def _twice(prod, w, h, variant, flags, forcing):
    """SPP samples, then MORE continued from the saved RNG streams (scan_checks.render_twice at this file's sample counts)."""
    f = rt.Film(w, h)
    st = f.render(prod, SPP, flags=flags, variant=variant, max_depth=DEPTH, **forcing)
    first = f.download().copy()
    st2 = f.render(prod, MORE, flags=flags | rt.FLAG_KEEP_RNG_STATE, variant=variant, max_depth=DEPTH, **forcing)
    return Scan(first, f.download().copy(), st.rays, st2.rays, st.kernel_kind, st.pixels_per_wave)


def _check(prod, w, h, forcings, want, rays=None, label=None):
    for forcing in forcings:
        for variant in (0, 1):
            got = _twice(prod, w, h, variant, 0, forcing)
            assert got.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
            for flags, what in REFERENCES:
                ref = _twice(prod, w, h, variant, flags, forcing)
                assert ref.kernel_kind == 16
                assert_same_scan(got, ref, (label, forcing, variant, what))
            if variant == 0:
                assert np.array_equal(got.first.view(np.uint64), want.view(np.uint64)), (label, forcing, "oracle")
                if rays is not None:
                    assert got.rays == rays, (label, forcing, "oracle's rays")


def _build(spheres, kw, w, h):
    return P.world(spheres, eye=kw.get("eye", P.EYE), look=kw.get("look", P.LOOK), vfov=kw.get("vfov", 50.0), aspect=w / h, glass=kw.get("glass", ()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_windows_and_queues_change_nothing(name):
    list_name, kw = CASES[name]
    spheres = LISTS[list_name]
    w, h = kw.get("width", L.W), kw.get("height", L.H)
    prod, orc = build_both(_build(spheres, kw, w, h))
    L.check_tables(spheres, prod, WINDOW_AXES[list_name])
    want, stats = orc.render(w, h, SPP, depth=DEPTH, want_stats=True)
    if kw.get("sky"):
        assert stats["rays"] == w * h * SPP, "every ray is a camera ray that leaves the scene"
    _check(prod, w, h, FORCINGS, want, stats["rays"], name)


@pytest.mark.parametrize("w, h", THIN_FRAMES)
@pytest.mark.parametrize("list_name", ["on_ground", "nested", "two_runs_general_between"])
def test_groups_left_without_a_ray(list_name, w, h):
    """3, 5 and 23 live lanes at the most: 4, 8 and 32 groups, of which 1, 3 and 9 and more hold the first ray's copy."""
    spheres = LISTS[list_name]
    prod, orc = build_both(_build(spheres, {}, w, h))
    want, stats = orc.render(w, h, SPP, depth=DEPTH, want_stats=True)
    _check(prod, w, h, [dict(coop_threshold=65)], want, stats["rays"], list_name)


def test_scene_11_as_a_list():
    w, h = 64, 48
    prod = rt.builtin_scene(11, 1, w, h)
    wins, _ = prod.scan_windows()
    assert [None if x is None else x[0] for x in wins] == [0, None]
    _check(prod, w, h, FORCINGS, Oracle().render(11, 1, w, h, SPP, depth=DEPTH), label="scene 11")
