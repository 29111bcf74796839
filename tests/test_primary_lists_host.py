"""The camera rays' candidate lists of the sphere-list kernel (csrc/primary_cull_rule.h) through rt_scene_dump_primary_lists,
without a device.

A tile's list must hold every sphere that any camera ray of any pixel of the tile could hit.  For each case the test restates
camera_ray in numpy from rt_scene_dump_camera and, for a few thousand rays per checked tile -- the tile's border pixels, jitter
at 0 and at 1, lens points on the rim and inside --, computes in fp64 every sphere whose line comes within r (1 + 1e-9) at some
t > 0: each must be listed, or the tile be marked "no list".  The converse keeps the rule from degenerating into "list everything":
no listed sphere is provably clear of the tile by the rule's own bound with one per cent added to every radius in it.  A list is
ascending and has no duplicates.

Also prints the histogram of list lengths of scene 11 at 1200 x 800 (profiles/r18_c2_list_lengths.txt): no number is fixed.
"""
import collections

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import primary_list_worlds as P


def _spheres_of(scene):
    """Centres and radii of a committed list world of static spheres, in list order, from its leaves' boxes."""
    kinds, boxes = scene.dump_leaves()
    assert len(kinds) == scene.info()["n_spheres"] and np.all(kinds == 0)
    return 0.5 * (boxes[:, 0::2] + boxes[:, 1::2]), 0.5 * (boxes[:, 1] - boxes[:, 0])


def _check(scene, centres, radii, width, height, tiles=None, stripe_rows=8, rank=0, world_size=1, seed=1, per_pixel=24):
    lists = scene.primary_lists(width, height, stripe_rows, rank, world_size)
    owned = rt.stripe_rows(height, stripe_rows, rank, world_size)
    assert len(lists) == ((width + 7) // 8) * ((len(owned) + 7) // 8)
    cam = P.Camera(scene.dump_camera())
    rnd = np.random.default_rng(seed)
    for tile in (range(len(lists)) if tiles is None else tiles):
        cols, rows = P.tile_pixels(tile, width, height, stripe_rows, rank, world_size)
        got = lists[tile]
        if got is None:
            continue
        assert got == sorted(set(got)) and len(got) <= 14 and all(0 <= k < len(radii) for k in got), (tile, got)
        o, d = P.tile_rays(cam, cols, rows, width, height, rnd, per_pixel)
        need = np.flatnonzero(P.reachable(o, d, centres, radii))
        assert set(need) <= set(got), (tile, "reachable but not listed", sorted(set(need) - set(got)), got)
        for k in got:
            assert not P.provably_clear(cam, cols, rows, width, height, centres[k], radii[k], 1.01), (tile, k, "listed, but clear of the tile by 1 %")
    return lists


@pytest.fixture(scope="module")
def scene11():
    s = rt.builtin_scene(11, 1, 1200, 800)
    return s, _spheres_of(s)


def _pixel_of(cam, point, width, height):
    """The pixel whose rays from the lens centre pass through `point`."""
    lam_s_t = np.linalg.solve(np.stack([point - cam.origin, -cam.horizontal, -cam.vertical], axis=1), cam.llc - cam.origin)
    return int(lam_s_t[1] * width), int(lam_s_t[2] * height)


def test_scene_11_corners_horizon_and_inside_the_glass_sphere(scene11):
    s, (centres, radii) = scene11
    lists = s.primary_lists(1200, 800)
    tiles_x, tiles_y = 150, 100
    ground = int(np.argmax(radii))
    glass = int(np.flatnonzero((np.abs(centres - np.array([0.0, 1.0, 0.0])).sum(axis=1) < 1e-12) & (radii == 1.0))[0])
    cam = P.Camera(s.dump_camera())
    gi, gj = _pixel_of(cam, centres[glass], 1200, 800)
    inside_glass = (gj // 8) * tiles_x + gi // 8
    assert lists[inside_glass] is not None and glass in lists[inside_glass]
    column = [lists[ty * tiles_x + 75] for ty in range(tiles_y)]
    sees_ground = [l is None or ground in l for l in column]
    horizon = next(ty for ty in range(1, tiles_y) if sees_ground[ty] != sees_ground[ty - 1])
    corners = [0, tiles_x - 1, (tiles_y - 1) * tiles_x, tiles_x * tiles_y - 1]
    _check(s, centres, radii, 1200, 800, tiles=corners + [horizon * tiles_x + 75, (horizon - 1) * tiles_x + 75, inside_glass], per_pixel=96)


def test_scene_11_list_lengths(scene11):
    s, _ = scene11
    lists = s.primary_lists(1200, 800)
    hist = collections.Counter("no list" if l is None else len(l) for l in lists)
    listed = [len(l) for l in lists if l is not None]
    print("\nscene 11 (485 spheres), 1200 x 800: %d tiles, list lengths:" % len(lists))
    for key in sorted(hist, key=lambda k: 99 if k == "no list" else k):
        print("  %7s: %5d tiles" % (key, hist[key]))
    print("  mean length of the %d listed tiles: %.3f" % (len(listed), float(np.mean(listed))))
    assert len(lists) == 15000


@pytest.mark.parametrize("stripe_rows, rank, world_size", [(8, 0, 1), (8, 1, 3), (5, 1, 3)])
def test_scene_11_at_61_by_45_every_tile(stripe_rows, rank, world_size):
    s = rt.builtin_scene(11, 1, 61, 45)
    centres, radii = _spheres_of(s)
    _check(s, centres, radii, 61, 45, stripe_rows=stripe_rows, rank=rank, world_size=world_size, per_pixel=8)


CASES = P.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_custom_worlds_every_tile(name):
    spheres, build = CASES[name]
    s = P.product(build)
    centres = np.array([c for c, _ in spheres], dtype=np.float64)
    radii = np.array([r for _, r in spheres], dtype=np.float64)
    lists = _check(s, centres, radii, P.W, P.H, per_pixel=8)
    last = len(spheres) - 1
    if name == "sky_only":
        assert all(l == [] for l in lists)
    if name == "camera_inside_glass" or name == "sphere_contains_lens":
        assert all(l is None or last in l for l in lists), "every ray starts inside that sphere"
    if name == "sphere_behind_camera":
        assert all(l is None or last not in l for l in lists), "a sphere wholly behind a pinhole camera is in no list"
    if name == "forty_in_a_row":
        centre = (P.NO_LIST_AT[1] // 8) * (P.W // 8) + P.NO_LIST_AT[0] // 8
        assert lists[centre] is None, "forty candidates do not fit a list"
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    assert lists[centre + dy * (P.W // 8) + dx] is not None, (dx, dy)
    if name == "coincident_pair":
        assert any(l is not None and 20 in l and 21 in l for l in lists)
