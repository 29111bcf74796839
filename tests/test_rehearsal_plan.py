"""The rehearsal's two plan fields (csrc/launch_plan.cpp plan_frame) through rt_plan_launch, without a GPU: probe_keeps -- the
frame launch resumes from the rehearsed samples instead of rendering them again -- and probe_ray_cap -- a rehearsed pixel stops
where its place on the longest-chain list is decided.  Over the plans of the benchmark frames and the boundary sizes of
tests/test_launch_plan.py, plain and adaptive; tests/test_rehearsal_keep_gpu.py renders what these plans describe."""
import os

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from test_launch_plan import plan


@pytest.fixture(scope="module")
def earth():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_stb.npz"))["bytes"]


def check(scene, w, h, spp, **kw):
    """The three rules, for a plain and an adaptive film; returns the plain plan."""
    plans = [plan(scene, w, h, spp, adaptive=adaptive, **kw) for adaptive in (False, True)]
    for adaptive, got in zip((False, True), plans):
        where = (w, h, spp, kw, adaptive)
        assert got["probe_keeps"] == (1 if got["probe_spp"] > 0 and not adaptive else 0), where
        capped = got["pixel_classes"] == 1 and got["super_threshold"] > 0
        assert got["probe_ray_cap"] == (got["super_threshold"] if capped else 0), where
        if got["probe_spp"] > 0:
            assert got["probe_spp"] < spp, where
    return plans[0]


def test_benchmark_frames(earth):
    c2 = check(rt.builtin_scene(11, 1, 1200, 800), 1200, 800, 500, variant=0)
    assert (c2["probe_spp"], c2["probe_keeps"], c2["probe_ray_cap"]) == (8, 1, 96)
    c3 = check(rt.builtin_scene(0, 0, 1200, 800), 1200, 800, 500, variant=0)
    assert (c3["probe_spp"], c3["probe_keeps"], c3["probe_ray_cap"]) == (8, 1, 240)
    c4 = check(rt.builtin_scene(7, 0, 800, 800), 800, 800, 1000, variant=1)
    assert (c4["probe_spp"], c4["probe_keeps"], c4["probe_ray_cap"]) == (8, 1, 0)      # ranking only: kept, no cap
    s = rt.builtin_scene(9, 0, 1600, 1600, earth=earth)
    c5 = check(s, 1600, 1600, 5000, variant=0)
    assert (c5["probe_spp"], c5["probe_keeps"], c5["probe_ray_cap"]) == (8, 1, 0)
    for rank in (0, 7):  # the deep kernel's classes have no list of the longest chains: no cap
        part = check(s, 1600, 1600, 200, variant=0, rank=rank, world_size=8)
        assert (part["pixel_classes"], part["super_threshold"], part["probe_keeps"], part["probe_ray_cap"]) == (1, 0, 1, 0)
    for w, h in ((768, 560), (768, 568), (768, 776), (1024, 968), (1344, 1024), (1344, 1032)):
        check(s, w, h, 200)
    check(s, 1600, 1600, 200, rank=0, world_size=8, num_cus=64)


def test_boundaries():
    s = rt.builtin_scene(11, 1, 256, 256)
    got = {}
    for w, h, spp in ((256, 256, 64), (256, 256, 63), (255, 257, 64), (255, 256, 64), (256, 256, 399), (256, 256, 400), (256, 256, 32),
                      (256, 256, 31), (248, 264, 500), (255, 257, 500), (248, 256, 500), (256, 248, 500)):
        got[w, h, spp] = check(s, w, h, spp)
    assert (got[256, 256, 64]["probe_keeps"], got[256, 256, 64]["probe_ray_cap"]) == (1, 48)
    assert (got[256, 256, 400]["probe_keeps"], got[256, 256, 400]["probe_ray_cap"]) == (1, 96)
    assert (got[256, 256, 63]["probe_keeps"], got[256, 256, 63]["probe_ray_cap"]) == (1, 0)
    assert (got[256, 256, 32]["probe_spp"], got[256, 256, 32]["probe_keeps"]) == (1, 1)     # a frame launch of 31
    assert (got[255, 257, 64]["probe_keeps"], got[255, 257, 64]["probe_ray_cap"]) == (1, 0)   # ranking only
    for none in ((256, 256, 31), (248, 264, 500), (248, 256, 500), (256, 248, 500)):
        assert (got[none]["probe_spp"], got[none]["probe_keeps"], got[none]["probe_ray_cap"]) == (0, 0, 0)
    for kw in (dict(flags=rt.FLAG_ROW_MAJOR_TILES), dict(flags=rt.FLAG_NO_PIXEL_CLASSES), dict(pixels_per_wave=8), dict(max_blocks_per_cu=1)):
        check(s, 256, 256, 500, **kw)
    twin = check(s, 256, 256, 500, flags=rt.FLAG_NO_PIXEL_CLASSES | rt.FLAG_ROW_MAJOR_TILES)
    assert (twin["probe_spp"], twin["probe_keeps"], twin["probe_ray_cap"]) == (0, 0, 0)
    box = rt.builtin_scene(7, 1, 64, 64)
    for ppw in (0, 63, 1):
        check(box, 64, 64, 8, pixels_per_wave=ppw)
