"""The launch plan (csrc/launch_plan.h) through rt_plan_launch, without a GPU: which kernel a launch runs and how its frame is
scheduled.  The frames are bit-identical whatever the plan decides, so no rendering test notices a wrong threshold or a wrong
fallback: these do.  Part (a) holds the plan to every kernel kind an existing GPU test pins for a scene, a world and its flags
(the tables and scene builders are those tests' own); part (b) to the plans of the benchmark frames on a GPU of 256 compute
units, field by field, and to the boundaries of the rules.  tests/test_launch_plan_gpu.py ties the plan to what ran."""
import os

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import test_adaptive_gpu as A
import test_motion_time_gpu as M
import test_shading_gpu as G
from frame_helpers import render_params
from test_custom_scenes_gpu import _deep_media_world
from test_motion_time import field

ADAPTIVE = 512
DEEP_LDS = 64 * 1024   # the general kernel's deep form stages more than this (kind 7 both ways)


@pytest.fixture(scope="module")
def earth():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_stb.npz"))["bytes"]


def plan(scene, w, h, spp, variant=0, flags=0, num_cus=256, adaptive=False, rank=0, world_size=1, coop_threshold=0,
         max_blocks_per_cu=0, pixels_per_wave=0):
    p = render_params(w, h, spp, rank=rank, world_size=world_size, variant=variant, flags=flags, coop_threshold=coop_threshold,
                      max_blocks_per_cu=max_blocks_per_cu, pixels_per_wave=pixels_per_wave)
    return scene.plan_launch(p, num_cus=num_cus, adaptive=adaptive)


def product(build):
    s = rt.Scene()
    build(s, rt.Rng)
    return s


# ---- (a) the kinds the GPU tests pin ----
def test_every_instantiation_of_the_adaptive_tests_table(earth):
    """test_adaptive_gpu.instantiation_cases: all fifteen (kind, deep) pairs, plain and with the adaptive bit; the five-wave
    build of the instanced list scan has no adaptive form, its frame goes to the four-wave build."""
    reached = set()
    for name, make, w, h, cap, tau, kw, kind, big in A.instantiation_cases(earth):
        scene = make()
        for variant in (0, 1):
            plain = plan(scene, w, h, cap, variant=variant, **kw)
            adapt = plan(scene, w, h, cap, variant=variant, adaptive=True, **kw)
            assert plain["kernel_kind"] == kind and adapt["kernel_kind"] == kind + ADAPTIVE, (name, plain["kernel_kind"], adapt["kernel_kind"])
            assert (kind == 7 and plain["lds_bytes"] > DEEP_LDS) == big, (name, plain["lds_bytes"])
            assert adapt["probe_kernel"] == plain["kernel"], name    # the rehearsal of an adaptive frame is the plain kernel's
            if "five-wave" in name:
                assert (plain["waves_per_simd"], adapt["waves_per_simd"]) == (5, 4)
            else:
                assert plain["lds_bytes"] == adapt["lds_bytes"] and plain["waves_per_simd"] == adapt["waves_per_simd"], name
        reached.add((kind, big))
    assert reached == A.ALL_KINDS


@pytest.mark.parametrize("texture", G.TEXTURES)
@pytest.mark.parametrize("world", ["list", "bvh"])
def test_textured_carriers(texture, world):
    for media in (True, False):
        s = product(G.carrier_world(texture, world, media=media))
        for variant in (0, 1):
            assert plan(s, G.W, G.H, 4, variant=variant)["kernel_kind"] == G.expected_kind(texture, world, media=media)


@pytest.mark.parametrize("texture", sorted(G.NESTED_FLOOR))
@pytest.mark.parametrize("world", ["list", "bvh"])
@pytest.mark.parametrize("tree", ["bvh_object", "instance_of_list"])
def test_nested_carriers(texture, world, tree):
    kind = 39 if (world == "bvh" and tree == "instance_of_list") else 47
    got = plan(product(G.carrier_world(texture, world, tree=tree)), G.W, G.H, 4)
    assert got["kernel_kind"] == kind
    # nested kernels are outside the scheduler's "BVH kernel" and "list kernel": no rehearsal at any frame size
    big = plan(product(G.carrier_world(texture, world, tree=tree)), 1200, 800, 500)
    assert big["kernel_kind"] == kind and (big["rank_tiles"], big["pixel_classes"], big["probe_spp"]) == (0, 0, 0)


@pytest.mark.parametrize("shape,world,flags,ppw,kind", G.INLINE_CASES)
def test_inline_texture_worlds(shape, world, flags, ppw, kind):
    s = product(G.inline_world(shape, world))
    got = plan(s, G.W, G.H, 6, flags=flags, pixels_per_wave=ppw)
    assert got["kernel_kind"] == kind and got["pixels_per_wave"] == ppw
    general = plan(s, G.W, G.H, 6, flags=flags | G.FLAG_FORCE_GENERAL, pixels_per_wave=ppw)
    assert general["kernel_kind"] & 1


def test_deep_rich_worlds():
    """Segmented walk 263 and, on the reference's tree, the deep general kernel (both compiled for three waves per SIMD, the
    general kernel for two); a third Perlin table does not fit the deep kernels' LDS: the general kernel, with little staged.
    Pixel classes for the deep kernels only with more than 64 KB staged (200 more boxes bring the rows there)."""
    two, three = product(G.deep_rich_world(2)), product(G.deep_rich_world(2, unused_noise=1))
    for variant in (0, 1):
        seg = plan(two, G.DEEP_W, G.DEEP_H, G.DEEP_SPP, variant=variant)
        ref = plan(two, G.DEEP_W, G.DEEP_H, G.DEEP_SPP, variant=variant, flags=G.FLAG_REFERENCE_TREE)
        assert seg["kernel_kind"] == 263 and seg["waves_per_simd"] == 3
        assert ref["kernel_kind"] == 7 and ref["waves_per_simd"] == 3
        for flags in (0, G.FLAG_REFERENCE_TREE):
            b = plan(three, G.DEEP_W, G.DEEP_H, 8, variant=variant, flags=flags)
            assert b["kernel_kind"] == 7 and b["lds_bytes"] < 32 * 1024 and b["waves_per_simd"] == 2
    filled = product(G.deep_rich_world(2, filler_boxes=200))
    for flags, kind in ((0, 263), (G.FLAG_REFERENCE_TREE, 7)):
        a = plan(filled, 256, 256, 64, flags=flags)
        b = plan(filled, 256, 256, 64, flags=flags | G.FLAG_NO_PIXEL_CLASSES)
        assert a["kernel_kind"] == b["kernel_kind"] == kind and a["lds_bytes"] > DEEP_LDS and a["waves_per_simd"] == 3
        assert (a["pixel_classes"], b["pixel_classes"]) == (1, 0)
        assert plan(two, 256, 256, 64, flags=flags)["pixel_classes"] == 0   # the same kernel with less than 64 KB staged: none


@pytest.mark.parametrize("scene", ["static", "moving", "inside", "mixed"])
def test_material_edge_worlds(scene):
    for world in ("list", "bvh"):
        s = product(G.edges_world(scene, world))
        assert plan(s, G.W, G.H, 8)["kernel_kind"] == G.EDGE_KINDS[scene, world]
        if world == "bvh":
            assert plan(s, G.W, G.H, 8, flags=G.FLAG_ALWAYS_WALK)["kernel_kind"] == G.EDGE_KINDS_WALKED[scene]
    if scene == "mixed":
        return
    for variant in (0, 1):
        s = product(G.edges_world(scene, "bvh"))
        others = [dict(flags=G.FLAG_ALWAYS_WALK), dict(flags=G.FLAG_ALWAYS_WALK | G.FLAG_REFERENCE_TREE), dict(flags=G.FLAG_FORCE_GENERAL),
                  dict(flags=G.FLAG_ALWAYS_WALK | G.FLAG_FORCE_GENERAL), dict(pixels_per_wave=8)]
        assert [plan(s, G.W, G.H, 8, variant=variant, **kw)["kernel_kind"] for kw in others] == [64, 0, 7, 7, 136]
        s = product(G.edges_world(scene, "list"))
        k0 = G.EDGE_KINDS[scene, "list"]
        others = [dict(flags=G.FLAG_EXACT_SCAN), dict(flags=G.FLAG_FILTER_FP64), dict(coop_threshold=65), dict(pixels_per_wave=8),
                  dict(flags=G.FLAG_FORCE_GENERAL)]
        assert [plan(s, G.W, G.H, 8, variant=variant, **kw)["kernel_kind"] for kw in others] == [k0] * 3 + [16 if k0 == 16 else 136, 15]


@pytest.mark.parametrize("case", M.IDS)
def test_shutter_and_moving_spheres(case):
    """test_motion_time_gpu (a), (c), (d), (f): a shutter that lets a moving sphere leave its box takes the reference's tree,
    walked, and ignores RT_FLAG_ACCELERATE_LISTS -- and switches the thin-wave scan of a sphere BVH world off."""
    motion, shutter, rise, inside = M.CASES[case]
    for variant in (0, 1):
        s = product(field("bvh", motion, shutter, rise=rise, moving_every=3, quads=True))
        got = plan(s, M.W, M.H, M.SPP, variant=variant)
        assert got["kernel_kind"] == (64 if inside else 0)
        assert (got["reference_tree"], got["always_walk"]) == ((0, 0) if inside else (1, 1))
        assert plan(s, M.W, M.H, M.SPP, variant=variant, flags=M.FLAG_REFERENCE_TREE)["kernel_kind"] == 0
        s = product(field("bvh", motion, shutter, rise=rise, moving_every=2))
        assert plan(s, M.W, M.H, M.SPP, variant=variant, coop_threshold=65)["coop_threshold"] == (65 if inside else 0)
        assert plan(s, M.W, M.H, M.SPP, variant=variant)["coop_threshold"] == 0
        s = product(field("bvh", motion, shutter, rise=rise, n=11))
        assert plan(s, M.W, M.H, M.SPP, variant=variant)["kernel_kind"] == (8 if inside else 0)
        assert plan(s, M.W, M.H, M.SPP, variant=variant, flags=M.FLAG_ALWAYS_WALK)["kernel_kind"] == (64 if inside else 0)
        s = product(field("list", motion, shutter, rise=rise, moving_every=3, quads=True))
        assert plan(s, M.W, M.H, M.SPP, variant=variant)["kernel_kind"] == 8
        accel = plan(s, M.W, M.H, M.SPP, variant=variant, flags=M.FLAG_ACCELERATE_LISTS)
        assert accel["kernel_kind"] == (64 if inside else 8) and accel["accelerate_lists"] == (1 if inside else 0)
        for ppw in (16, 1):
            assert plan(s, M.W, M.H, M.SPP, variant=variant, pixels_per_wave=ppw)["kernel_kind"] == 8 + 128
        if rise != 0.0:
            s = product(_deep_media_world(("mist", "ball", "crate"), motion=motion, shutter=shutter))
            got = plan(s, M.W, M.H, M.SPP, variant=variant, flags=M.FLAG_FORCE_GENERAL)
            ref = plan(s, M.W, M.H, M.SPP, variant=variant, flags=M.FLAG_FORCE_GENERAL | M.FLAG_REFERENCE_TREE)
            assert bool(got["kernel_kind"] & 256) == inside and not ref["kernel_kind"] & 256


def test_worlds_too_big_for_the_lds_only_kernels():
    """test_custom_scenes_gpu's two fall-backs, chosen by the plan: 600 moving spheres with a material each do not fit beside
    the library tree's node rows (400 do) -- the reference-tree kernel, and no accelerated list either; 700 boxes do not fit
    the deep kernels' LDS (500 do) -- the general kernel of two waves per SIMD."""
    def spheres(world, n):
        def build(s, Rng):
            rnd = np.random.default_rng(11)
            items = []
            for k in range(n):
                c = rnd.uniform(-6, 6, 3)
                c[2] -= 12.0
                mat = s.Lambertian(tuple(rnd.uniform(0.1, 0.9, 3))) if k % 3 else s.Metal(tuple(rnd.uniform(0.4, 0.9, 3)), 0.1)
                items.append(s.MovingSphere(tuple(c), tuple(c + np.array([0.0, 0.2, 0.0])), 0.0, 1.0, 0.25, mat))
            s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
            s.Camera((0, 0, 2), (0, 0, -12), (0, 1, 0), 50, 2.0, 0.0, 10.0, 0.0, 1.0)
            s.Commit()
        return product(build)

    def boxes(n):
        def build(s, Rng):
            rnd = np.random.default_rng(12)
            ground = s.Lambertian((0.48, 0.83, 0.53))
            items = []
            for k in range(n):
                x, z = (k % 28) * 1.0 - 14.0, (k // 28) * 1.0 - 30.0
                items.append(s.MakeBox((x, -2.0, z), (x + 0.9, -2.0 + float(rnd.uniform(0.1, 1.0)), z + 0.9), ground))
            items.append(s.Sphere((0, 1, -12), 1.5, s.Lambertian(s.NoiseTexture(0.2, Rng(1984, 5)))))
            items.append(s.Sphere((0, 8, -10), 2.0, s.DiffuseLight((7, 7, 7))))
            s.SetWorld(s.BvhNode(items))
            s.Camera((0, 2, 4), (0, 0, -12), (0, 1, 0), 50, 2.0, 0.0, 10.0, 0.0, 1.0, (0.1, 0.1, 0.1))
            s.Commit()
        return product(build)

    for n, kind in ((400, 64), (600, 0)):
        got = plan(spheres("bvh", n), 64, 32, 4)
        assert got["kernel_kind"] == kind and got["lds_nodes"] == 1
        assert (got["lds_bytes"] > DEEP_LDS) == (kind == 64)
        assert plan(spheres("list", n), 64, 32, 4, flags=rt.FLAG_ACCELERATE_LISTS)["kernel_kind"] == (64 if kind else 8)
    subset(plan(boxes(500), 64, 32, 4), kernel_kind=263, waves_per_simd=3)
    subset(plan(boxes(500), 64, 32, 4, flags=rt.FLAG_REFERENCE_TREE), kernel_kind=7, waves_per_simd=3)
    for flags in (0, rt.FLAG_REFERENCE_TREE):
        got = subset(plan(boxes(700), 64, 32, 4, flags=flags), kernel_kind=7, waves_per_simd=2)
        assert got["lds_bytes"] < DEEP_LDS


def test_builtin_scenes(earth):
    """test_parity_gpu and smoke(): scene 11 as a list is the sphere list (16), scene 0 the library's tree (64; 0 on the
    reference's), the Cornell box a list scan in both worlds (10), the Book-2 final scene the segmented walk (263)."""
    assert plan(rt.builtin_scene(11, 1, 48, 24), 48, 24, 2)["kernel_kind"] == 16
    assert plan(rt.builtin_scene(0, 0, 48, 24), 48, 24, 2)["kernel_kind"] == 64
    assert plan(rt.builtin_scene(0, 0, 48, 24), 48, 24, 2, flags=rt.FLAG_REFERENCE_TREE)["kernel_kind"] == 0
    assert plan(rt.builtin_scene(11, 1, 48, 24), 48, 24, 2, flags=rt.FLAG_ACCELERATE_LISTS)["kernel_kind"] == 64
    for world in (0, 1):
        assert plan(rt.builtin_scene(7, world, 48, 24), 48, 24, 2)["kernel_kind"] == 10
    assert plan(rt.builtin_scene(7, 0, 48, 24), 48, 24, 2, flags=rt.FLAG_ALWAYS_WALK)["kernel_kind"] == 2
    assert plan(rt.builtin_scene(9, 0, 48, 24, earth=earth), 48, 24, 2)["kernel_kind"] == 263


# ---- (b) the plans of the benchmark frames on 256 compute units ----
def subset(got, **want):
    assert {k: got[k] for k in want} == want
    return got


NO_CLASSES = dict(pixel_classes=0, heavy_threshold=0, super_threshold=0, near_percent=0, near_neighbours=0, heavy_waves=0, heavy_ppw=0,
                  super_ppw=0, heavy_priority=0, adaptive_ppw=0)


def test_c2_frame():
    """Sphere list, 1200 x 800 x 500, strict: tiles ranked; heavy pixels from 9 rays per sample of 8 rehearsed, the longest from
    12; two serving waves of eight / four pixels with priority; three workgroups per CU (the rehearsal: two)."""
    got = plan(rt.builtin_scene(11, 1, 1200, 800), 1200, 800, 500, variant=0)
    subset(got, kernel_kind=16, pixels_per_wave=64, rank_tiles=1, tile_flatness_x8=9, pixel_classes=1, probe_spp=8, heavy_threshold=72,
           super_threshold=96, near_percent=0, near_neighbours=0, heavy_waves=2, heavy_ppw=8, super_ppw=4, heavy_priority=3,
           max_blocks_per_cu=3, probe_max_blocks_per_cu=2, adaptive_ppw=0, coop_threshold=24, lds_spheres=1)
    assert got["kernel"] == got["probe_kernel"]


def test_c3_frame():
    """Random spheres with motion blur, BvhNode world, 1200 x 800 x 500: the library's tree with everything in LDS; heavy
    pixels from 9 rays per sample (or 70 % of that among three heavy neighbours), the longest (30) one to a wave."""
    got = plan(rt.builtin_scene(0, 0, 1200, 800), 1200, 800, 500, variant=0)
    subset(got, kernel_kind=64, pixels_per_wave=64, rank_tiles=1, tile_flatness_x8=9, pixel_classes=1, probe_spp=8, heavy_threshold=72,
           super_threshold=240, near_percent=70, near_neighbours=3, heavy_waves=3, heavy_ppw=6, super_ppw=1, heavy_priority=0,
           adaptive_ppw=0, coop_threshold=0, max_blocks_per_cu=0, lds_nodes=1, waves_per_simd=3)
    assert got["lds_bytes"] > DEEP_LDS


def test_c4_frame():
    """Cornell box with two instances, 800 x 800 x 1000, fast: 640 000 pixels are three generations on the lanes of four waves
    per SIMD and two on those of five, 3 > 2 x 1.38: the five-wave instantiation; tiles ranked, no classes."""
    got = plan(rt.builtin_scene(7, 0, 800, 800), 800, 800, 1000, variant=1)
    subset(got, kernel_kind=10, waves_per_simd=5, pixels_per_wave=64, rank_tiles=1, probe_spp=8, tile_flatness_x8=9, **NO_CLASSES)
    assert got["lds_bytes"] == 256 * (12 * 8 + 5 * 4)   # the parked path state and nothing else
    # a frame that does not fill the lanes of four waves stays there, and so does an adaptive one
    assert plan(rt.builtin_scene(7, 0, 800, 800), 512, 256, 1000, variant=1)["waves_per_simd"] == 4
    assert plan(rt.builtin_scene(7, 0, 800, 800), 800, 800, 1000, variant=1, adaptive=True)["waves_per_simd"] == 4


def test_c5_frame_and_one_rank_of_eight(earth):
    """Book-2 final scene, 1600 x 1600: the whole frame at 5000 spp is 13 generations of pixels per lane -- ranked tiles, no
    classes; one rank of eight at 200 spp is 1.6 -- classes from 8 rays per sample of 4 rehearsed, ten serving waves of 32
    pixels that take fewer where the lists are short."""
    s = rt.builtin_scene(9, 0, 1600, 1600, earth=earth)
    whole = plan(s, 1600, 1600, 5000, variant=0)
    subset(whole, kernel_kind=263, rank_tiles=1, probe_spp=8, tile_flatness_x8=9, node_burst=24, park_ratio=4, **NO_CLASSES)
    assert whole["lds_bytes"] > DEEP_LDS
    for rank in (0, 7):
        part = plan(s, 1600, 1600, 200, variant=0, rank=rank, world_size=8)
        subset(part, kernel_kind=263, rank_tiles=1, pixel_classes=1, probe_spp=4, heavy_threshold=32, super_threshold=0, heavy_waves=10,
               heavy_ppw=32, super_ppw=0, heavy_priority=0, adaptive_ppw=1, near_percent=0)
    # the three bands of the deep kernel's classes (generations of pixels per resident lane: up to 2.2, 5, 7) and beyond
    bands = [(768, 560, 8, 10, 1), (768, 568, 12, 6, 1), (768, 768, 12, 6, 1), (768, 776, 12, 6, 0), (1024, 960, 12, 6, 0),
             (1024, 968, 16, 4, 0), (1344, 1024, 16, 4, 0)]
    for w, h, rays, waves, fewer in bands:
        subset(plan(s, w, h, 200), pixel_classes=1, heavy_threshold=rays * 4, heavy_waves=waves, heavy_ppw=32, adaptive_ppw=fewer)
    subset(plan(s, 1344, 1032, 200), rank_tiles=1, probe_spp=2, **NO_CLASSES)
    # a smaller GPU holds fewer lanes: the same rank's share is more generations there
    subset(plan(s, 1600, 1600, 200, rank=0, world_size=8, num_cus=64), pixel_classes=1, heavy_threshold=16 * 4, heavy_waves=4, adaptive_ppw=0)


def test_boundaries():
    """63 / 64 samples and 65 535 / 65 536 pixels (classes), 31 / 32 samples and 1023 / 1024 tiles (ranking), 399 / 400
    samples (rehearsed samples), the flags that switch either off, pixels_per_wave given."""
    s = rt.builtin_scene(11, 1, 256, 256)
    subset(plan(s, 256, 256, 64), rank_tiles=1, pixel_classes=1, probe_spp=4, heavy_threshold=36, super_threshold=48, max_blocks_per_cu=3)
    subset(plan(s, 256, 256, 63), rank_tiles=1, probe_spp=1, max_blocks_per_cu=2, **NO_CLASSES)
    subset(plan(s, 255, 257, 64), rank_tiles=1, probe_spp=1, **NO_CLASSES)          # 65 535 pixels (1056 tiles): one short
    subset(plan(s, 255, 256, 64), rank_tiles=1, probe_spp=1, **NO_CLASSES)          # 65 280 pixels, 1024 tiles
    subset(plan(s, 256, 256, 399), pixel_classes=1, probe_spp=4)
    subset(plan(s, 256, 256, 400), pixel_classes=1, probe_spp=8, heavy_threshold=72)
    subset(plan(s, 256, 256, 32), rank_tiles=1, probe_spp=1)
    subset(plan(s, 256, 256, 31), rank_tiles=0, probe_spp=0, tile_flatness_x8=0)
    subset(plan(s, 248, 264, 500), rank_tiles=0, probe_spp=0, pixel_classes=0)      # 31 x 33 = 1023 tiles: one short
    subset(plan(s, 255, 257, 500), rank_tiles=1, pixel_classes=0, probe_spp=5)
    subset(plan(s, 248, 256, 500), rank_tiles=0, probe_spp=0, pixel_classes=0)      # 31 x 32 = 992 tiles
    subset(plan(s, 256, 248, 500), rank_tiles=0, probe_spp=0, pixel_classes=0)
    subset(plan(s, 256, 256, 500, flags=rt.FLAG_ROW_MAJOR_TILES), rank_tiles=0, pixel_classes=1, probe_spp=8)
    subset(plan(s, 256, 256, 500, flags=rt.FLAG_NO_PIXEL_CLASSES), rank_tiles=1, probe_spp=5, **NO_CLASSES)
    subset(plan(s, 256, 256, 500, flags=rt.FLAG_NO_PIXEL_CLASSES | rt.FLAG_ROW_MAJOR_TILES), rank_tiles=0, probe_spp=0, **NO_CLASSES)
    subset(plan(s, 256, 256, 500, pixels_per_wave=8), kernel_kind=16, pixels_per_wave=8, rank_tiles=1, **NO_CLASSES)
    subset(plan(s, 256, 256, 500, max_blocks_per_cu=1), pixel_classes=1, max_blocks_per_cu=1, probe_max_blocks_per_cu=1)
    # list scans deal lanes in powers of two; the sphere list takes any count
    box = rt.builtin_scene(7, 1, 64, 64)
    for given, used, kind in ((0, 64, 10), (64, 64, 10), (63, 32, 138), (3, 2, 138), (1, 1, 138)):
        subset(plan(box, 64, 64, 8, pixels_per_wave=given), pixels_per_wave=used, kernel_kind=kind, waves_per_simd=4 if kind == 10 else 3)
    subset(plan(s, 64, 64, 8, pixels_per_wave=3), pixels_per_wave=3, kernel_kind=16)


def test_shutter_that_leaves_a_moving_spheres_box_at_benchmark_size():
    """C3's world with the shutter open beyond the spheres' interval: the reference's tree, walked, no thin-wave scan, and none of
    the classes that only the library-tree kernel has -- the tiles are still ranked."""
    got = plan(product(field("bvh", (0.0, 1.0), (0.0, 3.0))), 1200, 800, 500, coop_threshold=17)
    subset(got, kernel_kind=0, reference_tree=1, always_walk=1, accelerate_lists=0, coop_threshold=0, rank_tiles=1, probe_spp=5, **NO_CLASSES)
    inside = plan(product(field("bvh", (0.0, 1.0), (0.0, 1.0))), 1200, 800, 500, coop_threshold=17)
    subset(inside, kernel_kind=64, reference_tree=0, always_walk=0, coop_threshold=17, rank_tiles=1, pixel_classes=1, probe_spp=8)
    small = plan(product(field("bvh", (0.0, 1.0), (0.0, 3.0), n=11)), 1200, 800, 500)
    subset(small, kernel_kind=0, always_walk=1)                                      # no scan of its twelve leaves either
    lst = plan(product(field("list", (0.0, 1.0), (0.0, 3.0))), 1200, 800, 500, flags=rt.FLAG_ACCELERATE_LISTS)
    subset(lst, kernel_kind=8, accelerate_lists=0, rank_tiles=1, **NO_CLASSES)


def test_refused_params():
    s = rt.builtin_scene(10, 0, 16, 8)
    for bad in (dict(pixels_per_wave=65), dict(world_size=2, rank=2), dict(num_cus=0)):
        with pytest.raises(rt.RtowError):
            plan(s, 16, 8, 1, **bad)
    with pytest.raises(rt.RtowError):
        plan(rt.Scene(), 16, 8, 1)   # not committed
