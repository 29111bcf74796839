"""Sphere-list scan (kernel kind 16): list lengths against the trip of the packed filter's loop.

The pixel-parallel scan reads the packed fp32 rows (flat_scene.h SphereScanPair) eight spheres per trip from a table that the host
pads to whole trips with rows that never pass, plus the two pairs the last trip reads ahead; the loop has no tail and no clamp.
These worlds walk the list length over every residue of the trip -- every length from 1 to two trips plus one -- and over 485
(the Book-1 world's own count) and 1300 (above the 1216 rows that fit the LDS planes, so the survivors' rows come from global
memory).  Each world is built so that a row lost or misplaced at the end of the table shows:

  * the LAST sphere is the ground, which most pixels see and which the fp32 filter does not decide (k = -inf: far outside the
    bulk; in lists of one or two spheres there is no bulk to be outside of and it is decided like any other), so the last trip
    always holds an undecided sphere, and behind it comes only the padding;
  * the sphere before it is a large one in the middle of the view, decided by the filter;
  * the camera sits near the world origin, where the centres of the padding rows lie.

For every length, both builds and both filter forms (packed fp32, the default, and RT_FLAG_FILTER_FP64) give the frame, the ray
count and the continued RNG streams of the exact scan (RT_FLAG_EXACT_SCAN); the strict build also equals the CPU oracle bit for bit.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import build_both
from scan_checks import SPP, assert_same_scan, assert_strict_equals_oracle, ground, render_twice, small_spheres

pytestmark = pytest.mark.gpu

W, H = 96, 64
TRIP = 8  # spheres per trip of the loop (render.hip kFilterTrip)
LENGTHS = list(range(1, 2 * TRIP + 2)) + [485, 1300]


def _world(n):
    def build(s, Rng):
        rnd = np.random.default_rng(1000 + n)
        items = small_spheres(s, rnd, max(0, n - 2))
        if n >= 2:
            items.append(s.Sphere((0.0, 0.6, -6.0), 1.2, s.Metal((0.8, 0.7, 0.6), 0.05)))
        items.append(ground(s))
        assert len(items) == n
        s.SetWorld(s.HittableList(items))
        s.Camera((0.0, 0.3, 0.5), (0.0, 0.0, -5.0), (0, 1, 0), 50, W / H, 0.0, 10.0)
        s.Commit()
    return build


def test_lengths_cover_the_trip():
    assert {n % TRIP for n in LENGTHS} == set(range(TRIP))
    assert set(range(1, 2 * TRIP + 2)) <= set(LENGTHS) and 485 in LENGTHS and max(LENGTHS) > 1216


@pytest.mark.parametrize("n", LENGTHS)
def test_every_list_length_equals_exact_scan_and_oracle(n):
    prod, orc = build_both(_world(n))
    want, stats = orc.render(W, H, SPP, want_stats=True)
    for variant in (0, 1):
        ref = render_twice(prod, W, H, variant, rt.FLAG_EXACT_SCAN)
        assert ref.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
        for flags in (0, rt.FLAG_FILTER_FP64):
            got = render_twice(prod, W, H, variant, flags)
            assert got.kernel_kind == 16
            assert_same_scan(got, ref, (n, variant, flags, "against the exact scan"))
        if variant == 0:
            assert_strict_equals_oracle(ref, want, stats)
