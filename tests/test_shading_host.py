"""The parts of the shading tests that need no GPU: the scenes of tests/test_shading_gpu.py commit in the host builder and
render on the oracle, their tables have the sizes the GPU tests rely on, boxes and leaf order equal the oracle's, bad
texture handles are refused, and every edge material of part 4 is really in view (swapping it changes the oracle's frame)."""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import OracleRng, OracleScene, build_both
import test_shading_gpu as G

W, H = G.W, G.H

SCENES = {}
for _t in G.TEXTURES:
    for _w in ("list", "bvh"):
        SCENES[f"carriers-{_t}-{_w}"] = (G.carrier_world(_t, _w), _t)
        SCENES[f"carriers-{_t}-{_w}-no-media"] = (G.carrier_world(_t, _w, media=False), _t)
for _t in sorted(G.NESTED_FLOOR):
    for _w in ("list", "bvh"):
        for _tree in ("bvh_object", "instance_of_list"):
            SCENES[f"nested-{_t}-{_tree}-{_w}"] = (G.carrier_world(_t, _w, tree=_tree), _t)
for _s in ("spheres", "prims", "instances", "media"):
    for _w in ("list", "bvh"):
        SCENES[f"inline-{_s}-{_w}"] = (G.inline_world(_s, _w), "plain")
for _s in ("static", "moving", "inside", "mixed"):
    for _w in ("list", "bvh"):
        SCENES[f"edges-{_s}-{_w}"] = (G.edges_world(_s, _w), "plain")
SCENES["deep-1"] = (G.deep_rich_world(1), "deep")
SCENES["deep-2"] = (G.deep_rich_world(2), "deep")
SCENES["deep-2+1"] = (G.deep_rich_world(2, unused_noise=1), "deep")
SCENES["deep-2-filler"] = (G.deep_rich_world(2, filler_boxes=200), "deep")


class Recording:
    """A scene whose BvhNode calls are written down as permutations of their arguments (handles differ between the two
    sides, positions do not)."""

    def __init__(self, scene):
        self._s, self.orders = scene, []

    def __getattr__(self, name):
        return getattr(self._s, name)

    def BvhNode(self, items):
        before = list(items)
        root = self._s.BvhNode(items)
        self.orders.append([before.index(h) for h in items])
        return root


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_commits_with_the_expected_tables_and_the_oracles_leaf_order(name):
    """Every scene of parts 1-4 commits without a GPU; info() reports the Perlin tables, images and image bytes the GPU
    tests count on (an unused NoiseTexture counts: 1, 2, 3); every BvhNode sorts its leaves as the oracle's does."""
    build, what = SCENES[name]
    prod, orc = Recording(rt.Scene()), Recording(OracleScene())
    build(prod, rt.Rng)
    build(orc, OracleRng)
    info = prod.info()
    if what in ("plain", "chk_solid", "chk_chk"):
        assert (info["n_perlin"], info["n_images"], info["image_bytes"]) == (0, 0, 0)
    elif what == "deep":
        assert info["n_perlin"] == {"deep-1": 1, "deep-2": 2, "deep-2+1": 3, "deep-2-filler": 2}[name]
        assert (info["n_images"], info["image_bytes"]) == (4, G.IMAGE_BYTES)
        assert info["n_nodes"] > 64 and info["n_media"] == 3
    else:   # four images with data and the cyan one, which has no bytes
        assert (info["n_perlin"], info["n_images"], info["image_bytes"]) == (1, 5, G.IMAGE_BYTES)
    assert prod.orders == orc.orders
    assert ("bvh" in name or what == "deep") == bool(prod.orders)


def test_image_sizes_and_offsets():
    """The largest image is not the first, so the images that matter start at a non-zero offset of the byte table."""
    sizes = [G.IMAGE_SIZES[n] for n in G.IMAGE_ORDER]
    assert sizes[0] != max(sizes, key=lambda s: s[0] * s[1]) and G.IMAGE_BYTES == 100434
    assert sorted(sizes) == [(1, 1), (2, 3), (37, 19), (256, 128)]


@pytest.mark.parametrize("texture", G.TEXTURES)
@pytest.mark.parametrize("world", ["list", "bvh"])
def test_carrier_scenes_are_about_their_texture_on_the_oracle(texture, world):
    """The condition the GPU test asserts as well, here without a GPU: image lookups, noise calls and medium draws are
    each at least 5 % of the rays in the scenes that are about them; and without media the oracle's own BVH world equals
    its list world."""
    orc = OracleScene()
    G.carrier_world(texture, world)(orc, OracleRng)
    frame, stats = orc.render(W, H, 4, want_stats=True)
    assert np.isfinite(frame).all()
    keys = G.about(texture)
    assert keys, texture
    for key in keys:
        assert stats[key] >= 0.05 * stats["rays"], (key, stats[key], stats["rays"])
    if world == "bvh":
        frames = []
        for w in ("list", "bvh"):
            o = OracleScene()
            G.carrier_world(texture, w, media=False)(o, OracleRng)
            frames.append(o.render(W, H, 4))
        assert np.array_equal(frames[0], frames[1])


def test_unused_noise_texture_leaves_the_oracles_frame_unchanged():
    a, b = OracleScene(), OracleScene()
    G.deep_rich_world(2)(a, OracleRng)
    G.deep_rich_world(2, unused_noise=1)(b, OracleRng)
    assert np.array_equal(a.render(G.DEEP_W, G.DEEP_H, 2), b.render(G.DEEP_W, G.DEEP_H, 2))
    one = OracleScene()
    G.deep_rich_world(1)(one, OracleRng)
    assert not np.array_equal(a.render(G.DEEP_W, G.DEEP_H, 2), one.render(G.DEEP_W, G.DEEP_H, 2)), "the second table must show"


def test_bounding_boxes_of_negative_radius_and_moving_spheres_equal_the_oracles():
    def build(s, Rng):
        m = s.Dielectric(1.5)
        return s, [s.Sphere((1, 2, 3), -0.5, m), s.Sphere((1, 2, 3), 0.5, m), s.Sphere((-300.0, 0.25, 1e3), -7.0, m),
                   s.MovingSphere((1.5, 1.8, 0.5), (1.5, 2.1, 0.5), 0.0, 1.0, -0.45, m),
                   s.MovingSphere((1.5, 1.8, 0.5), (1.5, 2.1, 0.5), 0.0, 1.0, 0.45, m),
                   s.MovingSphere((-1, 0, 0), (2, -3, 4), 0.25, 0.75, -1.25, m),
                   s.Translate(s.RotateY(s.Sphere((0.3, 0, 0), -0.7, m), -50.0), (2, 0.7, 2))]
    (p, hp), (o, ho) = build(rt.Scene(), rt.Rng), build(OracleScene(), OracleRng)
    for a, b in zip(hp, ho):
        assert p.BoundingBox(a) == o.BoundingBox(b)
    assert p.BoundingBox(hp[0]) == [0.5, 1.5, 1.5, 2.5, 2.5, 3.5] == p.BoundingBox(hp[1])


def test_invalid_texture_handles_are_refused():
    s = rt.Scene()
    good = s.SolidColor((0.5, 0.5, 0.5))
    ball = s.Sphere((0, 0, 0), 1.0, s.Dielectric(1.5))
    for bad in (0, good + 1, 9999, -1 & 0xFFFFFFFF):
        for make in (lambda t: s.Lambertian(int(t)), lambda t: s.DiffuseLight(int(t)), lambda t: s.Isotropic(int(t)),
                     lambda t: s.ConstantMedium(ball, 1.0, int(t)), lambda t: s.CheckerTexture(0.5, int(t), good),
                     lambda t: s.CheckerTexture(0.5, good, int(t))):
            with pytest.raises(rt.RtowError):
                make(bad)
    assert s.Lambertian(good) and s.DiffuseLight(good) and s.Isotropic(good) and s.ConstantMedium(ball, 1.0, good)


def test_oracle_refuses_an_image_it_has_no_room_for():
    """oracle_c_image keeps copies of at most 16 images; the 17th used to become the cyan fallback without a word."""
    o = OracleScene()
    px = np.full((2, 2, 3), 200, dtype=np.uint8)
    for _ in range(16):
        o.ImageTexture(px)
    with pytest.raises(AssertionError):
        o.ImageTexture(px)
    assert o.ImageTexture(None) > 0, "the image without data needs no copy"


def test_every_edge_material_decides_paths_on_the_oracle():
    """Non-vacuity of part 4: with any one edge material swapped for grey Lambertian, the oracle's frame of the scene
    differs in at least 1 % of the pixels -- the material is in view and decides paths."""
    def frame(swap):
        o = OracleScene()
        G.edges_world("moving", "list", swap=swap)(o, OracleRng)
        return o.render(W, H, 8)
    base = frame(None)
    assert np.isfinite(base).all() and base.max() > 1.0
    for k in range(G.N_EDGE_SWAPS):
        changed = float(np.mean(np.any(frame(k) != base, axis=-1)))
        assert changed >= 0.01, (k, changed)


def test_camera_inside_glass_is_a_different_population_of_paths():
    rays = {}
    for scene in ("static", "inside"):
        o = OracleScene()
        G.edges_world(scene, "list")(o, OracleRng)
        for depth in (50, 3):
            rays[scene, depth] = o.render(W, H, 8, depth=depth, want_stats=True)[1]["rays"]
    assert rays["inside", 50] > 1.3 * rays["static", 50] and rays["inside", 3] > 1.3 * rays["static", 3]
    assert rays["static", 3] < rays["static", 50] and rays["inside", 3] < rays["inside", 50]
