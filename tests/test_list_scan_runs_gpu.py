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

pytestmark = pytest.mark.gpu

W, H, SPP, MORE, DEPTH = S.W, S.H, 4, 2, 8
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


def _render_twice(prod, variant, flags):
    """SPP samples, then MORE from the saved RNG streams: the frame, the continued frame, the rays of both launches, the kernel, pixels per wave."""
    film = rt.Film(W, H)
    st = film.render(prod, SPP, max_depth=DEPTH, variant=variant, flags=flags)
    first = film.download().copy()
    st2 = film.render(prod, MORE, max_depth=DEPTH, variant=variant, flags=flags | rt.FLAG_KEEP_RNG_STATE)
    return first, film.download().copy(), st.rays, st2.rays, st.kernel_kind, st.pixels_per_wave


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
        exact = _render_twice(prod, variant, rt.FLAG_EXACT_SCAN)
        fp64 = _render_twice(prod, variant, rt.FLAG_FILTER_FP64)
        got = _render_twice(prod, variant, 0)
        assert exact[4] == 16 and fp64[4] == 16 and got[4] == 16, "a list of spheres is rendered by the sphere-list kernel"
        # one lane per ray: every wave begins with 64 live lanes, above the cooperative scan's threshold, so at least the camera
        # rays of every pixel go through the pixel-parallel scan -- the packed loop under test when no scan flag is set
        assert got[5] == 64 and exact[5] == 64 and fp64[5] == 64
        for ref, what in ((exact, "exact scan"), (fp64, "fp64 filter")):
            assert got[2] == ref[2] and got[3] == ref[3], (name, variant, what, "ray counts differ")
            assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), (name, variant, what)
            assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), (name, variant, what, "continued streams")
        if variant == 0:
            assert got[2] == stats["rays"]
            assert np.array_equal(got[0].view(np.uint64), want.view(np.uint64))
