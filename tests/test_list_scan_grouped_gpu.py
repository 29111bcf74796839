"""Sphere-list scan (kernel kind 16): the grouped scan, which deals a thin wave's L rays to groups of g = 64 / m lanes.

Lane s of a group puts spheres s, s + g, s + 2g, ... of its ray through the conservative filter, four to a batch, and runs the
reference's test on those that pass, each against the closest hit the ones before left it; one reduction per group over (t, index)
then picks the hit the sequential scan returns.  The grouped scan serves the waves that hold few rays, so the tests force it:

  * coop_threshold = 65 sends every pass through it: up to 64 rays to a wave (g = 1) on the 96 x 64 frame, and on frames of
    3 x 1, 5 x 1 and 23 x 1 pixels L = 3, 5 and up to 23 rays (g = 16, 8, down to 2; L no power of two), on 8 x 3 pixels 24 and
    fewer as the pixels end (g = 2);
  * pixels_per_wave = 1 ... 32 gives every ray g = 64 ... 2 lanes.

Worlds: a string of 40 overlapping spheres along the view axis, interleaved with a loose field (a central ray passes them all: at
g = 1 its lane has 40 survivors in a row and at g = 2 some lane at least 17, so every slot of many consecutive batches is taken and
each test starts from the hit of the one before); coincident spheres with different materials at list positions that fall to one
lane of a group and to different lanes for g = 2, 8 and 16 (the lowest index wins every tie, R/HittableList.h); spheres far outside
the bulk (ground-sphere size) first, in the middle, last and two within one batch of four; and list lengths at the batch edges of
g = 16 and g = 8, 485 (the Book-1 count) and 1300, above the 1216 rows of the LDS planes, where the planes are not staged and the
one-ray cooperative scan answers.

For every world and forcing, both builds and both filter forms (flags 0 and RT_FLAG_FILTER_FP64) give the frame, both ray counts
and the continued RNG streams of RT_FLAG_EXACT_SCAN under the same forcing; the strict build also equals the CPU oracle bit for bit.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import build_both
from scan_checks import SPP, assert_same_scan, assert_strict_equals_oracle, ground, material, render_twice, small_spheres

pytestmark = pytest.mark.gpu

W, H = 96, 64
FORCINGS = [dict(coop_threshold=65)] + [dict(pixels_per_wave=p) for p in (1, 2, 4, 8, 16, 32)]
LENGTHS = [1, 2, 63, 64, 65, 127, 129, 485, 1300]
THIN_FRAMES = [(3, 1), (5, 1), (23, 1), (8, 3)]
A_AT, B_AT = (5, 6, 13, 21, 37), (15, 16, 31, 32)  # list positions of the coincident copies (_coincident_world)
FROM, AT = np.array((0.0, 0.8, 1.0)), np.array((0.0, 0.3, -5.0))


def _finish(s, items, w, h):
    s.SetWorld(s.HittableList(items))
    s.Camera(tuple(FROM), tuple(AT), (0, 1, 0), 45, w / h, 0.0, 10.0)
    s.Commit()


def _string_world(w=W, h=H):
    def build(s, Rng):
        rnd = np.random.default_rng(43)
        items = small_spheres(s, rnd, 37)
        axis = (AT - FROM) / np.linalg.norm(AT - FROM)
        for k in range(40):  # one field sphere after every eight of the string
            c = FROM + (3.0 + 0.3 * k) * axis + np.array((0.02 * (k % 3), 0.0, 0.0))
            items.insert(2 + k + k // 8, s.Sphere(tuple(float(x) for x in c), 0.3, material(s, rnd, k + 1)))
        items.append(ground(s))
        _finish(s, items, w, h)
    return build


def _coincident_world():
    def build(s, Rng):
        rnd = np.random.default_rng(47)
        field = small_spheres(s, rnd, 44)
        mats = [s.Lambertian((0.8, 0.2, 0.2)), s.Metal((0.2, 0.8, 0.2), 0.0), s.Lambertian((0.2, 0.2, 0.8))]
        # List positions of the copies.  From the first copy of sphere A at 5: 6 is another lane for every g, 13 the same lane
        # for g = 2 and 8 and another for 16, 21 and 37 the same lane for all three.  Sphere B's first copy sits in the LAST lane
        # of a group of 8 or 16 (15), the next in the first lane of the next batch (16), then 31 and 32 likewise: the reduction
        # must prefer the lower index from the higher lane.  Sphere C is the first of the list and the last but one.
        a, b, c = ((0.0, 0.4, -4.0), 0.8), ((1.6, 0.5, -4.5), 0.6), ((-1.6, 0.5, -4.5), 0.6)
        copies = {k: (a, j) for j, k in enumerate(A_AT)}
        copies.update({k: (b, j + 1) for j, k in enumerate(B_AT)})
        copies[0] = (c, 2)
        items = []
        while field or len(items) in copies:
            if len(items) in copies:
                (centre, radius), j = copies[len(items)]
                items.append(s.Sphere(centre, radius, mats[j % 3]))
            else:
                items.append(field.pop())
        assert len(items) == 44 + len(copies)
        items.append(s.Sphere(c[0], c[1], mats[0]))
        items.append(ground(s))
        _finish(s, items, W, H)
    return build


def _undecided_world():
    def build(s, Rng):
        rnd = np.random.default_rng(41)
        items = small_spheres(s, rnd, 37)
        items.insert(0, ground(s))                                                            # first
        items.insert(17, s.Sphere((0.0, 0.0, 1006.0), 1000.0, s.Metal((0.8, 0.8, 0.9), 0.1)))  # 17 and 18: one batch of four
        items.insert(18, s.Sphere((-1006.0, 0.0, -5.0), 1000.0, s.Lambertian((0.7, 0.2, 0.2))))
        items.insert(len(items) // 2, s.Sphere((0.0, 1012.0, -5.0), 1000.0, s.Lambertian((0.6, 0.7, 0.9))))  # middle
        items.append(s.Sphere((1010.0, 0.0, -5.0), 1000.0, s.Lambertian((0.2, 0.2, 0.7))))    # last
        _finish(s, items, W, H)
    return build


def _length_world(n):
    def build(s, Rng):
        rnd = np.random.default_rng(2000 + n)
        items = small_spheres(s, rnd, max(0, n - 2))
        if n >= 2:
            items.append(s.Sphere((0.0, 0.6, -6.0), 1.2, s.Metal((0.8, 0.7, 0.6), 0.05)))
        items.append(ground(s))
        assert len(items) == n
        _finish(s, items, W, H)
    return build


def _check(build, forcings, w=W, h=H):
    prod, orc = build_both(build)
    want, stats = orc.render(w, h, SPP, want_stats=True)
    for forcing in forcings:
        for variant in (0, 1):
            ref = render_twice(prod, w, h, variant, rt.FLAG_EXACT_SCAN, render=forcing)
            assert ref.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
            for flags in (0, rt.FLAG_FILTER_FP64):
                got = render_twice(prod, w, h, variant, flags, render=forcing)
                assert got.kernel_kind == 16
                assert_same_scan(got, ref, (forcing, variant, flags, "against the exact scan"))
            if variant == 0:
                assert_strict_equals_oracle(ref, want, stats, label=forcing)


def test_positions_of_the_coincident_spheres_cover_same_and_other_lanes():
    first = A_AT[0]
    for g in (2, 8, 16):
        assert (A_AT[1] - first) % g != 0 and all((k - first) % g == 0 for k in A_AT[3:])
    assert (A_AT[2] - first) % 8 == 0 and (A_AT[2] - first) % 16 != 0
    for g in (8, 16):  # the lower index in the last lane of a group, the higher in the first
        assert all(k % g == g - 1 for k in B_AT[0::2]) and all(k % g == 0 for k in B_AT[1::2])


@pytest.mark.parametrize("world", ["string", "coincident", "undecided"])
def test_grouped_scan_equals_exact_scan_and_oracle(world):
    _check({"string": _string_world(), "coincident": _coincident_world(), "undecided": _undecided_world()}[world], FORCINGS)


@pytest.mark.parametrize("n", LENGTHS)
def test_grouped_scan_at_every_list_length(n):
    _check(_length_world(n), FORCINGS)


@pytest.mark.parametrize("w,h", THIN_FRAMES)
def test_grouped_scan_with_a_few_rays_to_the_wave(w, h):
    _check(_string_world(w, h), [dict(coop_threshold=65)], w, h)
