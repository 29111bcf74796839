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

pytestmark = pytest.mark.gpu

W, H, SPP, MORE = 96, 64, 4, 2
TRIP = 8  # spheres per trip of the loop (render.hip kFilterTrip)
LENGTHS = list(range(1, 2 * TRIP + 2)) + [485, 1300]


def _material(s, rnd, k):
    if k % 7 == 0:
        return s.Dielectric(1.5)
    if k % 3 == 0:
        return s.Metal(tuple(rnd.uniform(0.4, 0.9, 3)), float(rnd.uniform(0.0, 0.3)))
    return s.Lambertian(tuple(rnd.uniform(0.1, 0.9, 3)))


def _world(n):
    def build(s, Rng):
        rnd = np.random.default_rng(1000 + n)
        items = []
        for k in range(max(0, n - 2)):  # a loose field of small spheres in front of the camera
            c = (float(rnd.uniform(-3, 3)), float(rnd.uniform(-0.4, 1.2)), float(rnd.uniform(-9, -3)))
            items.append(s.Sphere(c, float(rnd.uniform(0.15, 0.45)), _material(s, rnd, k)))
        if n >= 2:
            items.append(s.Sphere((0.0, 0.6, -6.0), 1.2, s.Metal((0.8, 0.7, 0.6), 0.05)))
        items.append(s.Sphere((0.0, -1000.5, -5.0), 1000.0, s.Lambertian((0.5, 0.5, 0.5))))
        assert len(items) == n
        s.SetWorld(s.HittableList(items))
        s.Camera((0.0, 0.3, 0.5), (0.0, 0.0, -5.0), (0, 1, 0), 50, W / H, 0.0, 10.0)
        s.Commit()
    return build


def _render_twice(prod, variant, flags):
    """SPP samples, then MORE from the saved RNG streams: the frame, the rays of both launches and the continued frame."""
    film = rt.Film(W, H)
    st = film.render(prod, SPP, variant=variant, flags=flags)
    first = film.download().copy()
    st2 = film.render(prod, MORE, variant=variant, flags=flags | rt.FLAG_KEEP_RNG_STATE)
    return first, film.download().copy(), st.rays, st2.rays, st.kernel_kind


def test_lengths_cover_the_trip():
    assert {n % TRIP for n in LENGTHS} == set(range(TRIP))
    assert set(range(1, 2 * TRIP + 2)) <= set(LENGTHS) and 485 in LENGTHS and max(LENGTHS) > 1216


@pytest.mark.parametrize("n", LENGTHS)
def test_every_list_length_equals_exact_scan_and_oracle(n):
    prod, orc = build_both(_world(n))
    want, stats = orc.render(W, H, SPP, want_stats=True)
    for variant in (0, 1):
        ref = _render_twice(prod, variant, rt.FLAG_EXACT_SCAN)
        assert ref[4] == 16, "a list of spheres is rendered by the sphere-list kernel"
        for flags in (0, rt.FLAG_FILTER_FP64):
            got = _render_twice(prod, variant, flags)
            assert got[4] == 16
            assert got[2] == ref[2] and got[3] == ref[3], (n, variant, flags, "ray counts differ from the exact scan")
            assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), (n, variant, flags)
            assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), (n, variant, flags, "continued streams")
        if variant == 0:
            assert ref[2] == stats["rays"]
            assert np.array_equal(ref[0].view(np.uint64), want.view(np.uint64))
