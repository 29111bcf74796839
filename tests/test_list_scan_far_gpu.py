"""Sphere-list scan (kernel kind 16): the grouped scan where near and far spheres, list order and empty groups could matter.

The grouped scan (tests/test_list_scan_grouped_gpu.py) deals L rays to m >= L groups of lanes, and a group that is left without
a ray scans the wave's first ray once more, for a result nobody reads (csrc/render.hip scan_grouped; L = 3, 5 and up to 23 on the
thin frames below, and whatever is left as the pixels of a wave end).  The worlds were drawn up for a test that skips spheres wholly beyond a hit the ray has already
reached -- measured on the benchmark scene, it had next to nothing to skip and is not in the library (DESIGN.md section 5 "(r26)") --
and are kept as worlds in which any pruning by distance, by list order or by group would show, each under the forcings that send
every pass through the grouped scan (coop_threshold = 65; pixels_per_wave = 1 ... 32, i.e. g = 64 ... 2 lanes a ray).

  * the string of 40 overlapping spheres along the view axis, seen from both ends: the nearest sphere is the first of the string
    in list order, or the last, so the closest hit is met at once or only at the end;
  * a large sphere first in the list that is most rays' closest hit, with small spheres at its surface all around, in the
    same batch and in later ones: near roots a little in front of the large sphere's hit, a little beyond it and, on the far
    side, well beyond it;
  * small spheres behind a large one in the middle of the list, first and last in the list and partly hidden by it;
  * the camera inside a glass sphere and inside an opaque one, so that every sphere's centre lies within a radius of the first
    rays' origin along the ray, and glass spheres in the field, whose refracted rays start on a surface from inside;
  * coincident spheres at the list positions of tests/test_list_scan_grouped_gpu.py (one lane of a group, and different lanes,
    for g = 2, 8 and 16), seen with the list and against it: the lowest index wins every tie;
  * spheres the filter does not decide (ground-sized) first, in the middle and last, seen from both sides;
  * a field sorted by x seen along +x and along -x (with the list and against it), and the shuffled field of the other worlds;
  * lists of 63, 64, 65 and 485 rows.
Rays of zero length come from the scatter guards at the library's default depth of 50, as in the other scan tests.

For every world and forcing, both builds give the frame, both ray counts and the continued RNG streams of RT_FLAG_EXACT_SCAN and
of RT_FLAG_FILTER_FP64 (whose code is as it was) under the same forcing; the strict build also equals the CPU oracle bit for bit.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import build_both
from scan_checks import SPP, assert_same_scan, assert_strict_equals_oracle, ground, material, render_twice, small_spheres

pytestmark = pytest.mark.gpu

W, H = 96, 64
FORCINGS = [dict(coop_threshold=65)] + [dict(pixels_per_wave=p) for p in (1, 4, 8, 16, 32)]
THIN_FRAMES = [(3, 1), (5, 1), (23, 1)]
A_AT, B_AT = (5, 6, 13, 21, 37), (15, 16, 31, 32)  # as in tests/test_list_scan_grouped_gpu.py, which explains them
FROM, AT = np.array((0.0, 0.8, 1.0)), np.array((0.0, 0.3, -5.0))
AXIS = (AT - FROM) / np.linalg.norm(AT - FROM)
BACK = FROM + 18.0 * AXIS  # beyond the far end of the string, looking back at FROM


def _finish(s, items, w=W, h=H, view=(FROM, AT)):
    s.SetWorld(s.HittableList(items))
    s.Camera(tuple(float(x) for x in view[0]), tuple(float(x) for x in view[1]), (0, 1, 0), 45, w / h, 0.0, 10.0)
    s.Commit()


def _string_world(view, w=W, h=H):
    def build(s, Rng):
        rnd = np.random.default_rng(43)
        items = small_spheres(s, rnd, 37)
        for k in range(40):  # in list order from FROM outwards; one field sphere after every eight of the string
            c = FROM + (3.0 + 0.3 * k) * AXIS + np.array((0.02 * (k % 3), 0.0, 0.0))
            items.insert(2 + k + k // 8, s.Sphere(tuple(float(x) for x in c), 0.3, material(s, rnd, k + 1)))
        items.append(ground(s))
        _finish(s, items, w, h, view)
    return build


def _surface_world():
    def build(s, Rng):
        rnd = np.random.default_rng(53)
        centre, radius = np.array((0.0, 0.5, -4.5)), 1.2
        items = [s.Sphere(tuple(centre), radius, s.Lambertian((0.7, 0.6, 0.5)))]  # first: the largest radius and, for most rays, the closest hit
        def satellite(k):
            n = rnd.normal(size=3)
            n /= np.linalg.norm(n)
            c = centre + (radius + rnd.uniform(-0.1, 0.25)) * n  # half buried ... floating just off the surface, all around
            return s.Sphere(tuple(float(x) for x in c), 0.15, material(s, rnd, k + 1))
        items += [satellite(k) for k in range(6)]  # the large sphere's own batch
        items += small_spheres(s, rnd, 60)
        items += [satellite(k) for k in range(6, 54)]  # later batches: the large sphere has been met by then
        items.append(ground(s))
        _finish(s, items)
    return build


def _behind_world():
    def build(s, Rng):
        rnd = np.random.default_rng(59)
        centre, radius = np.array((0.2, 0.6, -4.0)), 1.5
        away = (centre - FROM) / np.linalg.norm(centre - FROM)
        side = np.cross(away, (0.0, 1.0, 0.0))
        def hidden(j):  # behind the large sphere, from its axis out past its limb
            c = centre + (radius + 0.4 + 0.3 * (j % 3)) * away + (0.35 * j - 1.4) * side
            return s.Sphere(tuple(float(x) for x in c), 0.1 + 0.02 * j, material(s, rnd, j + 1))
        items = [hidden(j) for j in range(4)] + small_spheres(s, rnd, 36)
        items.append(s.Sphere(tuple(centre), radius, s.Metal((0.8, 0.8, 0.8), 0.0)))  # position 40
        items += small_spheres(s, rnd, 30) + [ground(s)] + [hidden(j) for j in range(4, 9)]
        _finish(s, items)
    return build


def _inside_world(glass):
    def build(s, Rng):
        rnd = np.random.default_rng(61)
        items = small_spheres(s, rnd, 70)
        shell = s.Dielectric(1.5) if glass else s.Lambertian((0.8, 0.8, 0.3))
        items.insert(33, s.Sphere(tuple(float(x) for x in FROM + np.array((0.1, -0.05, 0.05))), 0.7, shell))  # the camera is inside
        items.insert(7, s.Sphere((0.0, 0.4, -4.0), 1.0, s.Dielectric(1.5)))  # bounce rays leave it from inside
        items.append(ground(s))
        _finish(s, items)
    return build


def _coincident_world(view):
    def build(s, Rng):
        rnd = np.random.default_rng(47)
        field = small_spheres(s, rnd, 44)
        mats = [s.Lambertian((0.8, 0.2, 0.2)), s.Metal((0.2, 0.8, 0.2), 0.0), s.Lambertian((0.2, 0.2, 0.8))]
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
        items.append(s.Sphere(c[0], c[1], mats[0]))
        items.append(ground(s))
        _finish(s, items, view=view)
    return build


def _undecided_world(view):
    def build(s, Rng):
        rnd = np.random.default_rng(41)
        items = small_spheres(s, rnd, 37)
        items.insert(0, ground(s))                                                            # first
        items.insert(17, s.Sphere((0.0, 0.0, 1006.0), 1000.0, s.Metal((0.8, 0.8, 0.9), 0.1)))  # 17 and 18: one batch of four
        items.insert(18, s.Sphere((-1006.0, 0.0, -5.0), 1000.0, s.Lambertian((0.7, 0.2, 0.2))))
        items.insert(len(items) // 2, s.Sphere((0.0, 1012.0, -5.0), 1000.0, s.Lambertian((0.6, 0.7, 0.9))))  # middle
        items.append(s.Sphere((1010.0, 0.0, -5.0), 1000.0, s.Lambertian((0.2, 0.2, 0.7))))    # last
        _finish(s, items, view=view)
    return build


def _sorted_world(sign):
    def build(s, Rng):
        rnd = np.random.default_rng(67)
        spheres = []
        for k in range(120):
            c = (float(rnd.uniform(-6, 6)), float(rnd.uniform(-0.3, 0.9)), float(rnd.uniform(-1.5, 1.5)))
            spheres.append((c, float(rnd.uniform(0.15, 0.45)), k))
        spheres.sort(key=lambda e: e[0][0])  # the list runs along +x
        items = [s.Sphere(c, r, material(s, rnd, k)) for c, r, k in spheres]
        items.append(s.Sphere((0.0, -1000.5, 0.0), 1000.0, s.Lambertian((0.5, 0.5, 0.5))))
        _finish(s, items, view=(np.array((-9.0 * sign, 0.6, 0.2)), np.array((0.0, 0.3, 0.0))))
    return build


def _length_world(n):
    def build(s, Rng):
        rnd = np.random.default_rng(3000 + n)
        items = small_spheres(s, rnd, n - 2)
        items.insert(n // 3, s.Sphere((0.0, 0.6, -6.0), 1.2, s.Metal((0.8, 0.7, 0.6), 0.05)))
        items.append(ground(s))
        assert len(items) == n
        _finish(s, items)
    return build


WORLDS = {
    "string, with the list": lambda: _string_world((FROM, AT)),
    "string, against the list": lambda: _string_world((BACK, FROM)),
    "satellites at a large sphere's surface": _surface_world,
    "small spheres behind a large one": _behind_world,
    "camera inside a glass sphere": lambda: _inside_world(True),
    "camera inside an opaque sphere": lambda: _inside_world(False),
    "coincident, with the list": lambda: _coincident_world((FROM, AT)),
    "coincident, from behind": lambda: _coincident_world((np.array((0.0, 0.8, -11.0)), AT)),
    "undecided, from the front": lambda: _undecided_world((FROM, AT)),
    "undecided, from behind": lambda: _undecided_world((np.array((0.0, 0.8, -11.0)), AT)),
    "sorted by x, seen along +x": lambda: _sorted_world(1.0),
    "sorted by x, seen along -x": lambda: _sorted_world(-1.0),
}


def _check(build, forcings, w=W, h=H):
    prod, orc = build_both(build)
    want, stats = orc.render(w, h, SPP, want_stats=True)
    for forcing in forcings:
        for variant in (0, 1):
            got = render_twice(prod, w, h, variant, 0, render=forcing)
            assert got.kernel_kind == 16, "a list of spheres is rendered by the sphere-list kernel"
            for flags in (rt.FLAG_EXACT_SCAN, rt.FLAG_FILTER_FP64):
                ref = render_twice(prod, w, h, variant, flags, render=forcing)
                assert ref.kernel_kind == 16
                assert_same_scan(got, ref, (forcing, variant, flags, "against the exact scan or the fp64 filter"))
            if variant == 0:
                assert_strict_equals_oracle(got, want, stats, label=forcing)


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_grouped_scan_finds_the_closest_hit(world):
    _check(WORLDS[world](), FORCINGS)


@pytest.mark.parametrize("n", [63, 64, 65, 485])
def test_grouped_scan_at_list_lengths(n):
    _check(_length_world(n), FORCINGS)


@pytest.mark.parametrize("w,h", THIN_FRAMES)
@pytest.mark.parametrize("view", ["with", "against"])
def test_grouped_scan_with_groups_left_empty(view, w, h):
    _check(_string_world((FROM, AT) if view == "with" else (BACK, FROM), w, h), [dict(coop_threshold=65)], w, h)
