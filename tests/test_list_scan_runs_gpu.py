"""Sphere-list scan (kernel kind 16): the shared-coordinate form of the packed filter's loop against the exact scan.

The host cuts the trips of the packed fp32 table into segments (tests/test_scan_segments_host.py) and the pixel-parallel scan
runs every run segment through a loop that forms the shared coordinate's terms once per ray (render.hip scan_filtered32,
filter_pairs<true>).  The filter only rejects and its survivors go through the reference's test, so frames do not change: for the
lists of the host test -- a run on each axis, runs entered and left off trip boundaries, general trips before, between and behind
runs, an undecided sphere and the padding inside a run -- and for a list just over the cap of the LDS sphere planes (survivors'
rows from global memory), both builds give the frame, the ray count and the continued RNG streams of RT_FLAG_EXACT_SCAN and of
RT_FLAG_FILTER_FP64; the strict build also equals the CPU oracle bit for bit.  64 x 48, 4 samples, depth 8.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import scan_segment_lists as S
from conftest import build_both
from scan_checks import SPP, assert_same_scan, assert_strict_equals_oracle, render_twice

pytestmark = pytest.mark.gpu

W, H, DEPTH = S.W, S.H, 8
LDS_SPHERE_CAP = 1216  # rows that fit the LDS planes of the sphere-list kernel (tests/test_list_scan_lengths_gpu.py)


def _over_the_cap():
    """1220 spheres: general trips, a run on y from row 16 to the padded end; the survivors' rows come from global memory."""
    rnd = np.random.default_rng(77)
    n = LDS_SPHERE_CAP + 4
    spheres = S.field(rnd, 16) + S.field(rnd, n - 16, y=0.3)
    return spheres, [(0, 16, None), (16, (n + S.TRIP - 1) // S.TRIP * S.TRIP - 16, 1)]


def _cases():
    cases = {name: (spheres, [(f, r, a) for f, r, a, _ in want]) for name, (spheres, want) in S.CASES.items()}
    cases["over_the_lds_cap"] = _over_the_cap()
    return cases


CASES = _cases()


def test_lists_are_small_and_one_is_over_the_cap():
    sizes = {name: len(spheres) for name, (spheres, _) in CASES.items()}
    assert all(40 <= n <= 80 for name, n in sizes.items() if name != "over_the_lds_cap"), sizes
    assert sizes["over_the_lds_cap"] > LDS_SPHERE_CAP


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_segments_equal_exact_scan_fp64_filter_and_oracle(name):
    spheres, want_segments = CASES[name]
    prod, orc = build_both(S.world(spheres))
    segs = prod.scan_segments()
    S.check_segments(spheres, segs)
    assert [(f, r, a) for f, r, a, _ in segs] == want_segments, "the list does not exercise the segments it is meant to"
    want, stats = orc.render(W, H, SPP, depth=DEPTH, want_stats=True)
    for variant in (0, 1):
        exact = render_twice(prod, W, H, variant, rt.FLAG_EXACT_SCAN, depth=DEPTH)
        fp64 = render_twice(prod, W, H, variant, rt.FLAG_FILTER_FP64, depth=DEPTH)
        got = render_twice(prod, W, H, variant, 0, depth=DEPTH)
        for r in (exact, fp64, got):
            assert r.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
            # one lane per ray: every wave begins with 64 live lanes, above the cooperative scan's threshold, so at least the
            # camera rays of every pixel go through the pixel-parallel scan -- the packed loop under test when no scan flag is set
            assert r.pixels_per_wave == 64
        for ref, what in ((exact, "exact scan"), (fp64, "fp64 filter")):
            assert_same_scan(got, ref, (name, variant, what))
        if variant == 0:
            assert_strict_equals_oracle(got, want, stats)
