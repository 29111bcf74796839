"""Ties between box faces, instances and resting spheres -- CPU side (the oracle, the host flattener, the launch plan).

Three things, none of which needs a GPU:
  (1) the worlds of tests/tie_worlds.py can see a wrong order: reversing the tied pair in the oracle's LIST render changes at
      least 0.5 % of the pixels, five times what the GPU tests' `within >= 0.999` may leave out -- a condition on the inputs,
      computed with the oracle alone (so that tests/test_tie_worlds_gpu.py cannot pass vacuously);
  (2) the oracle's BVH frame is one of the two list frames (which one is printed);
  (3) csrc/scene_builder.cpp has_coincident_primitives sees these ties -- no library tree, no segmented walk, no sub-BVH over
      them -- and leaves the worlds without a reachable tie their accelerators.
"""
import os

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import tie_worlds as T
from conftest import OracleRng, OracleScene
from frame_helpers import render_params
from test_custom_scenes_gpu import _deep_media_world

MIN_SHARE = 0.005
TYING = [p for p in T.PAIRS if T.PAIRS[p][0]]


def oracle_frame(build):
    orc = OracleScene()
    build(orc, OracleRng)
    return orc.render(T.W, T.H, T.SPP)


def product(build):
    s = rt.Scene()
    build(s, rt.Rng)
    return s


def kind(scene, flags=0, w=T.W, h=T.H, spp=T.SPP, pixels_per_wave=64):
    return scene.plan_launch(render_params(w, h, spp, flags=flags, pixels_per_wave=pixels_per_wave))["kernel_kind"]


# ---- (1), (2): the premise, with the oracle alone ----
@pytest.mark.parametrize("side", sorted(T.SIDES))
@pytest.mark.parametrize("pair", sorted(T.PAIRS))
def test_the_order_of_the_pair_decides_pixels_and_the_bvh_frame_is_one_of_the_two(pair, side):
    a = oracle_frame(T.tie_world(pair, "list", False, side=side))
    b = oracle_frame(T.tie_world(pair, "list", True, side=side))
    share = T.differing(a, b)
    bvh = oracle_frame(T.tie_world(pair, "bvh", False, side=side))
    from_a, from_b = T.differing(bvh, a), T.differing(bvh, b)
    print(f"{pair} {side}: the order decides {share:.4f} of the pixels; BVH frame differs from list order A in {from_a:.4f}, "
          f"from B in {from_b:.4f} -> equals {'A' if from_a == 0.0 else ('B' if from_b == 0.0 else 'neither')}")
    if T.PAIRS[pair][0]:
        assert share >= MIN_SHARE
    else:
        assert share == 0.0, "a moving sphere with time0 == time1 is never hit: nothing ties"
    assert from_a == 0.0 or from_b == 0.0


@pytest.mark.parametrize("twin", ["static", "resting"])
def test_the_order_inside_a_group_decides_pixels(twin):
    a = oracle_frame(T.group_world(twin, "list", False))
    b = oracle_frame(T.group_world(twin, "list", True))
    print(f"group with a {twin} twin: the order decides {T.differing(a, b):.4f} of the pixels")
    assert T.differing(a, b) >= MIN_SHARE
    assert T.differing(oracle_frame(T.group_world("none", "list", False)), oracle_frame(T.group_world("none", "list", True))) == 0.0


@pytest.mark.parametrize("pair", [p for p in T.COMPOSITE if p != "twin_boxes"])
def test_the_library_tree_would_separate_the_pair(pair):
    """Two leaves in one bottom node of the library's tree are tested in list order whatever the octant, and no walk can get
    their tie wrong.  With one of the pair moved by 2^-10 nothing ties, the world gets its tree, and the tree holds the two in
    different bottom nodes: the order in which a walk of it meets them depends on the ray's octant.  (The same world is the
    control of the guard: without the tie it keeps the segmented walk.)"""
    for fillers in (72, 6):
        build = T.tie_world(pair, "bvh", fillers=fillers, untied=True)
        s = product(build)
        assert T.separated_by_the_library_tree(s, build), (pair, fillers)
    deep = product(T.tie_world(pair, "bvh", untied=True))
    assert kind(deep, T.FLAG_FORCE_GENERAL) == 263
    a = oracle_frame(T.tie_world(pair, "list", False, untied=True))
    b = oracle_frame(T.tie_world(pair, "list", True, untied=True))
    assert T.differing(a, b) == 0.0, "moved apart, the order of the pair decides nothing"


# ---- (3) the guard ----
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("pair", TYING)
def test_a_tie_world_gets_no_tree_of_the_librarys_own(pair, swap):
    """Deep worlds: the reference's tree in the reference's order (kinds 7 and 0), never the segmented walk (263) or the library's
    tree (64); list worlds ignore RT_FLAG_ACCELERATE_LISTS; with a ball of fog beside the pair likewise."""
    for side in T.SIDES:   # (the camera does not enter the guard: one plan for all four)
        s = product(T.tie_world(pair, "bvh", swap, side=side))
        assert s.dump_fast_nodes()[0].shape[0] == 0, (pair, side)
        assert s.info()["n_nodes"] > 64
        if T.PAIRS[pair][1] == "plane":
            assert [kind(s, f) for f in (T.FLAG_FORCE_GENERAL, T.FLAG_FORCE_GENERAL | T.FLAG_REFERENCE_TREE)] == [7, 7]
        else:
            assert [kind(s, f) for f in (0, T.FLAG_REFERENCE_TREE, T.FLAG_FORCE_GENERAL)] == [0, 0, 7]
    lst = product(T.tie_world(pair, "list", swap))
    assert lst.dump_fast_nodes()[0].shape[0] == 0
    assert kind(lst, T.FLAG_ACCELERATE_LISTS) == kind(lst) == (10 if T.PAIRS[pair][1] == "plane" else 8)
    fog = product(T.tie_world(pair, "bvh", swap, media=True))
    assert fog.dump_fast_nodes()[0].shape[0] == 0 and kind(fog, T.FLAG_FORCE_GENERAL) == 7


def test_a_stopped_clock_ties_with_nothing():
    """time0 == time1: the moving sphere's centre is inf / NaN at every time, it is never hit -- the world keeps its tree."""
    s = product(T.tie_world("stopped_clock", "bvh"))
    assert s.dump_fast_nodes()[0].shape[0] > 0 and kind(s) == 64
    assert kind(product(T.tie_world("stopped_clock", "list")), T.FLAG_ACCELERATE_LISTS) == 64


def test_a_group_with_a_twin_gets_no_sub_bvh():
    nodes = {twin: product(T.group_world(twin, "list")).info()["n_nodes"] for twin in ("static", "resting", "none", "resting_apart")}
    print(nodes)
    assert nodes["static"] == nodes["resting"] == 0
    assert nodes["none"] > 0 and nodes["resting_apart"] > 0   # a resting moving sphere alone takes the sub-BVH from no group


# ---- controls: no reachable tie, accelerators kept ----
def test_the_final_scene_keeps_the_segmented_walk():
    earth = np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_stb.npz"))["bytes"]
    s = rt.builtin_scene(9, 0, 64, 64, earth=earth)
    assert s.dump_fast_nodes()[0].shape[0] > 0 and kind(s, w=64, h=64) == 263


def test_deep_media_world_keeps_the_segmented_walk():
    s = product(_deep_media_world(("mist", "ball", "crate")))
    assert kind(s, T.FLAG_FORCE_GENERAL, w=64, h=32, spp=6) == 263


@pytest.mark.parametrize("name", ["abutting_boxes", "separate_tops"])
def test_boxes_side_by_side_keep_the_segmented_walk(name):
    """Faces that abut with a solid on either side, coplanar tops and bottoms that share an edge at most: no ray sees a tie."""
    worlds = [getattr(T, name)("bvh")] + ([T.abutting_boxes("bvh", scale=0.7)] if name == "abutting_boxes" else [])
    for build in worlds:   # (scale 0.7: corners that are not dyadic, edge vectors fl(mx - mn) that do not add up exactly)
        s = product(build)
        assert s.info()["n_nodes"] > 64 and s.dump_fast_nodes()[0].shape[0] > 0
        assert kind(s, T.FLAG_FORCE_GENERAL) == 263


def test_abutting_glass_boxes_do_not():
    """The exemption is for materials that send no ray inwards: a ray inside one glass box leaves it into the next one."""
    def build(s, Rng):
        glass, red = s.Dielectric(1.5), s.Lambertian((0.8, 0.1, 0.1))
        items = [s.MakeBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), glass), s.MakeBox((1.0, 0.0, 0.0), (2.0, 1.0, 1.0), glass),
                 s.MakeBox((-2.0, 0.0, 0.0), (-1.0, 1.0, 1.0), red)]
        T._finish(s, items + T._fillers(s, 72), "bvh", "+z")
    s = product(build)
    assert s.dump_fast_nodes()[0].shape[0] == 0 and kind(s, T.FLAG_FORCE_GENERAL) == 7


def test_a_lone_resting_sphere_keeps_the_library_tree():
    s = product(T.lone_resting_sphere("bvh"))
    assert s.dump_fast_nodes()[0].shape[0] > 0 and kind(s) == 64
    assert kind(product(T.lone_resting_sphere("list")), T.FLAG_ACCELERATE_LISTS) == 64
