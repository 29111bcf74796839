"""Sphere-list scan (kernel kind 16): the survivor path of the conservative filter on lists shaped to stress it.

The filter runs one wave-level test per four spheres and then the behind-the-origin test and the queue append only for the
spheres some lane of the wave passed.  These worlds put the spheres the filter cannot decide (k = -inf: far outside the bulk,
like the Book-1 ground sphere) in other places of the list than the first, string spheres along the view axis so that a central
ray passes about 17 of the first 40 (more than the 8 a lane may hold before the scan drains its queue mid-list; the API does not
report drains, so this rests on the geometry), and repeat coincident spheres (the lowest index must win the tie as in R/HittableList.h).  For every world,
both builds and both filter forms (packed fp32, the default, and RT_FLAG_FILTER_FP64) give the frame, the ray count and the
continued RNG streams of the exact scan (RT_FLAG_EXACT_SCAN); the strict build also equals the CPU oracle bit for bit.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import build_both
from scan_checks import SPP, assert_same_scan, assert_strict_equals_oracle, ground, material, render_twice, small_spheres

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _world(where):
    def build(s, Rng):
        rnd = np.random.default_rng(41)
        items = small_spheres(s, rnd, 37)
        if where == "middle":
            items.insert(len(items) // 2, ground(s))
        elif where == "end":
            items.append(ground(s))
        elif where == "several":
            # four spheres far outside the bulk, spread over the list: two of them in one group of four
            items.insert(3, ground(s))
            items.insert(17, s.Sphere((0.0, 0.0, 1006.0), 1000.0, s.Metal((0.8, 0.8, 0.9), 0.1)))
            items.insert(18, s.Sphere((-1006.0, 0.0, -5.0), 1000.0, s.Lambertian((0.7, 0.2, 0.2))))
            items.append(s.Sphere((1010.0, 0.0, -5.0), 1000.0, s.Lambertian((0.2, 0.2, 0.7))))
        elif where == "cluster":
            # 24 spheres strung along the view axis and interleaved with the field: a central ray passes them all, and
            # more than 8 before the end of the list, so its queue is drained mid-scan
            for k in range(24):
                items.insert(k + 2 * (k % 6), s.Sphere((0.02 * (k % 3), 0.3, -3.0 - 0.35 * k), 0.3, material(s, rnd, k + 1)))
            items.append(ground(s))
        elif where == "coincident":
            # the same sphere three times in a row, then twice more further down, with different materials:
            # the lowest index wins every tie (R/HittableList.h keeps the first closest hit)
            mats = [s.Lambertian((0.8, 0.2, 0.2)), s.Metal((0.2, 0.8, 0.2), 0.0), s.Lambertian((0.2, 0.2, 0.8))]
            for j, at in enumerate((5, 6, 7, 22, 30)):
                items.insert(at, s.Sphere((0.0, 0.4, -4.0), 0.8, mats[j % 3]))
            items.insert(0, ground(s))
        s.SetWorld(s.HittableList(items))
        s.Camera((0.0, 0.8, 1.0), (0.0, 0.3, -5.0), (0, 1, 0), 45, W / H, 0.0, 10.0)
        s.Commit()
    return build


@pytest.mark.parametrize("where", ["middle", "end", "several", "cluster", "coincident"])
def test_filtered_scan_equals_exact_scan_and_oracle(where):
    prod, orc = build_both(_world(where))
    want, stats = orc.render(W, H, SPP, want_stats=True)
    for variant in (0, 1):
        ref = render_twice(prod, W, H, variant, rt.FLAG_EXACT_SCAN)
        assert ref.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
        for flags in (0, rt.FLAG_FILTER_FP64):
            got = render_twice(prod, W, H, variant, flags)
            assert got.kernel_kind == 16
            assert_same_scan(got, ref, (variant, flags, "against the exact scan"))
        if variant == 0:
            assert_strict_equals_oracle(ref, want, stats)
