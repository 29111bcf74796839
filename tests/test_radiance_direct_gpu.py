"""Radiance queries with light samples on the device (rt_scene_radiance_direct, Scene.radiance(direct="mis")): the estimator of
PathBatch(direct="mis").run(max_depth) in one launch.  Without lights, or with one bounce, it is Scene.radiance bit for bit; one
sample is the batch bit for bit; several samples are rounds of host path_advance_direct calls with the streams carried from round
to round; the stream continues across calls and may be written over its input; the mean estimates what Scene.radiance estimates
in both builds; and the executable prints what the call returns."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

import test_path_advance_direct_gpu as pad   # its worlds, rays and helpers, as they are
from conftest import ROOT
from light_worlds import no_lights_world
from query_helpers import bits, centre_rays

pytestmark = pytest.mark.gpu

N = pad.N   # 1000 rays: four workgroups, the last one partial
ALL = ("radiance", "path_rays", "rng_state")


def lamp_scene_in_a_tree():
    """pad.lamp_scene's four leaves under a BvhNode: the kernel's other instantiation."""
    s = rt.Scene()
    floor = s.Lambertian(s.CheckerTexture(0.5, s.SolidColor((0.8, 0.8, 0.8)), s.SolidColor((0.3, 0.5, 0.7))))
    items = [s.Quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), floor), s.Quad(*pad.LAMP, s.DiffuseLight((8.0, 8.0, 8.0))),
             s.Sphere(*pad.BALL, s.DiffuseLight((10.0, 6.0, 3.0))), s.Quad(*pad.SHADE, s.Lambertian((0.5, 0.5, 0.5)))]
    s.SetWorld(s.BvhNode(items))
    s.Camera((0, 1, 6), (0, 1, 0), (0, 1, 0), 40.0, 1.0, 0.0, 6.0, background=(0, 0, 0))
    s.Commit()
    return s


WORLDS = {
    "lamp scene": lambda: pad.world("lamp scene"),
    "lamp scene in a tree": lamp_scene_in_a_tree,
    "spheres": lambda: pad.world("spheres"),
    "moving spheres": lambda: pad.world("moving spheres"),
    "300 lights over a floor": lambda: pad.world("300 lights over a floor"),
    "lamp scene with fog": lambda: pad.lamp_scene(fog=True),
}


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


def first_rays():
    r = pad.rays()
    return r["origin"], r["direction"], r["time"], r["rng_state"]


def direct(scene, samples, depth, strategy=1, variant=0, states=None, want=ALL, stats=True):
    o, d, tm, first_states = first_rays()
    return scene.radiance(o, d, times=tm, rng_state=first_states if states is None else states, samples=samples, max_depth=depth,
                          variant=variant, want=want, stats=stats, direct="mis", strategy=strategy)


# ---- 1. without lights, or with one bounce, it is the plain call ----
@pytest.mark.parametrize("name,depth", [("no lights", 5), ("lamp scene", 1), ("lamp scene in a tree", 1)])
def test_without_light_samples_it_is_the_plain_call_bit_for_bit(name, depth):
    scene = no_lights_world() if name == "no lights" else world(name)
    o, d, tm, states = first_rays()
    plain, plain_st = scene.radiance(o, d, times=tm, rng_state=states, samples=3, max_depth=depth, want=ALL, stats=True)
    for strategy in (0, 1):
        got, st = direct(scene, 3, depth, strategy)
        for k in ALL:
            assert np.array_equal(bits(got[k]), bits(plain[k])), (k, strategy)
        assert st.rays == plain_st.rays == int(plain["path_rays"].sum()) and st.shadow_rays == 0 and st.shadow_reached == 0
    assert (plain["path_rays"] >= 3).all()
    if name == "no lights":   # (a grey ball before a black sky: the searches and the streams are what can differ)
        assert plain["path_rays"].max() > 3, "some paths bounce"
    else:
        assert plain["radiance"].any()


def test_depth_zero_is_black_and_draws_nothing():
    o, d, tm, states = first_rays()
    got, st = direct(world("lamp scene"), 2, 0)
    assert not got["radiance"].any() and not got["path_rays"].any() and np.array_equal(got["rng_state"], states)
    assert st.rays == 0 and st.shadow_rays == 0


# ---- 2. one sample is the batch ----
@pytest.mark.parametrize("depth", [2, 6])
@pytest.mark.parametrize("name,strategy", [(name, 1) for name in sorted(WORLDS)] + [("lamp scene", 0), ("300 lights over a floor", 0)])
def test_one_sample_is_the_batch_bit_for_bit(name, strategy, depth):
    scene = world(name)
    o, d, tm, states = (pad.to_device(a) for a in first_rays())
    batch = rt.PathBatch(scene, o, d, times=tm, rng_state=states, direct="mis", strategy=strategy)
    want = batch.run(depth, check_every=0).cpu().numpy()
    got, st = direct(scene, 1, depth, strategy)
    assert np.array_equal(bits(got["radiance"]), bits(want))
    assert want.any() and (want >= 0).all()
    assert st.shadow_rays > 100, "shadow rays were cast"
    assert 0 < st.shadow_reached <= st.shadow_rays, "and some reached their lamp"
    assert st.rays == int(got["path_rays"].sum()) and (got["path_rays"] >= 1).all() and got["path_rays"].max() <= depth
    assert st.kernel_vgprs > 0 and st.seconds > 0.0


def test_the_worlds_of_test_2_have_what_it_says():
    assert world("lamp scene").info()["world_kind"] != world("lamp scene in a tree").info()["world_kind"], "both instantiations run"
    assert len(world("300 lights over a floor").lights()["kind"]) == 300 > pad.CAP, "rows beyond the part staged on chip"
    assert world("lamp scene with fog").info()["n_media"] == 1 and world("lamp scene").info()["n_media"] == 0


# ---- 3. several samples: rounds of host calls, the streams carried ----
def one_round(scene, states, depth, strategy):
    """One sample of every ray as a loop of host path_advance_direct calls from the first rays with the streams ``states``:
    (acc, the stream of every row after its path, its path searches, shadow rays cast, shadow rays that reached their lamp)."""
    o, d, tm, _ = first_rays()
    live = dict(origin=o, direction=d, time=tm, rng_state=states, throughput=np.ones((N, 3)), ray_id=np.arange(N, dtype=np.int32),
                scatter_pdf=np.zeros(N))
    acc = np.zeros((N, 3))
    after = np.zeros((N, 6), dtype=np.uint32)
    searches = np.zeros(N, dtype=np.uint32)
    cast = reached = 0
    for bounce in range(depth):
        if not len(live["ray_id"]):
            break
        # an ended row draws only what the step draws: its stream is path_step's
        step = scene.path_step(live["origin"], live["direction"], times=live["time"], rng_state=live["rng_state"], want=("status", "rng_state"))
        ended = step["status"] != 2
        after[live["ray_id"][ended]] = step["rng_state"][ended]
        searches[live["ray_id"]] += 1
        got, st = pad.advance(scene, live, acc, strategy, bounce < depth - 1, stats=True)
        assert len(got["ray_id"]) == int((~ended).sum())
        cast += st.shadow_rays
        reached += st.shadow_reached
        live = pad.contiguous(got)
    after[live["ray_id"]] = live["rng_state"]   # cut by the depth: the last call's output
    return acc, after, searches, cast, reached


@functools.lru_cache(maxsize=None)
def rounds(name, count, depth, strategy=1):
    scene = world(name)
    states = first_rays()[3]
    out = []
    for _ in range(count):
        acc, states, searches, cast, reached = one_round(scene, states, depth, strategy)
        out.append(dict(acc=acc, rng_state=states, path_rays=searches, cast=cast, reached=reached))
    return out


def mean_of(accs):
    total = np.zeros((N, 3))
    for acc in accs:
        total = total + acc
    return (1.0 / len(accs)) * total


@pytest.mark.parametrize("name", ["lamp scene", "lamp scene with fog"])
def test_several_samples_are_rounds_of_host_calls(name):
    want = rounds(name, 4, 4)[:3]
    got, st = direct(world(name), 3, 4)
    assert np.array_equal(bits(got["radiance"]), bits(mean_of([r["acc"] for r in want])))
    assert np.array_equal(got["path_rays"], sum(r["path_rays"] for r in want))
    assert np.array_equal(got["rng_state"], want[-1]["rng_state"])
    assert st.rays == int(got["path_rays"].sum())
    assert st.shadow_rays == sum(r["cast"] for r in want) > 100 and st.shadow_reached == sum(r["reached"] for r in want) > 0


# ---- 4. continuation and aliasing ----
def test_the_stream_continues_and_may_be_written_over_its_input():
    scene, want = world("lamp scene"), rounds("lamp scene", 4, 4)
    whole, _ = direct(scene, 4, 4)
    assert np.array_equal(bits(whole["radiance"]), bits(mean_of([r["acc"] for r in want])))
    assert np.array_equal(whole["rng_state"], want[3]["rng_state"])
    first, _ = direct(scene, 2, 4)
    assert np.array_equal(first["rng_state"], want[1]["rng_state"])
    second, _ = direct(scene, 2, 4, states=np.ascontiguousarray(first["rng_state"]))
    assert np.array_equal(second["rng_state"], whole["rng_state"]), "one call of 4 samples, or two of 2"
    assert np.array_equal(bits(second["radiance"]), bits(mean_of([r["acc"] for r in want[2:]]))), "samples 3 and 4"
    # the torch path: the numpy path's bits
    o, d, tm, states = (pad.to_device(a) for a in first_rays())
    dev = scene.radiance(o, d, times=tm, rng_state=states, samples=2, max_depth=4, want=ALL, direct="mis", strategy=1)
    for k in ALL:
        assert np.array_equal(bits(pad.to_host(k, dev[k]).view(first[k].dtype)), bits(first[k])), k
    # rng_state out is the input array (the device call: the host call stages its arrays apart)
    radiance = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    p = _lib.RadianceDirectParams(N, 2, 4, 0.0, 0, 0, 0, 0, None, (C.c_int32 * 4)(), 1)
    rays = _lib.RadianceRays(o.data_ptr(), d.data_ptr(), tm.data_ptr(), states.data_ptr())
    out = _lib.RadianceOut(radiance.data_ptr(), None, states.data_ptr())
    assert api.lib().rt_scene_radiance_direct_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), None) == 0, api.lib().rt_last_error()
    assert np.array_equal(pad.to_host("rng_state", states), first["rng_state"])
    assert np.array_equal(bits(radiance.cpu().numpy()), bits(first["radiance"]))


# ---- 5. the estimator, both builds ----
@functools.lru_cache(maxsize=None)
def plain_means():
    o, d = pad.floor_points()
    scene = pad.lamp_scene()
    return np.stack([scene.radiance(o, d, samples=pad.SAMPLES, max_depth=2, seed=100, first_sequence=64 * b)["radiance"] for b in range(pad.BATCHES)])


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_the_mean_estimates_what_radiance_estimates(variant):
    """Scene.radiance(max_depth=2) against Scene.radiance(direct="mis", max_depth=2) on the scene, the 64 points, the 16 batches and
    the 4096 samples a point of test_path_advance_direct_gpu's estimator check: within 5 combined standard errors at every point and
    channel, the combined standard error of the lit points under 2 % of their mean."""
    o, d = pad.floor_points()
    scene = pad.lamp_scene()
    A = plain_means()
    M = np.stack([scene.radiance(o, d, samples=pad.SAMPLES, max_depth=2, seed=300, first_sequence=64 * b, variant=variant, direct="mis",
                                 strategy=1)["radiance"] for b in range(pad.BATCHES)])
    (a, sa), (m, sm) = pad.mean_se(A), pad.mean_se(M)
    lit = a.sum(axis=1) > 0.0
    combined = np.sqrt(sa ** 2 + sm ** 2)
    print("lit points", int(lit.sum()), "mean A", a[lit].mean(), "se A", sa[lit].mean(), "se M", sm[lit].mean(), "combined / mean",
          combined[lit].mean() / a[lit].mean(), "max |A-M| / se", np.nanmax(np.abs(a - m)[lit] / combined[lit]))
    assert np.all(np.abs(a - m) <= 5.0 * combined)
    assert combined[lit].mean() <= 0.02 * a[lit].mean()
    assert lit.sum() >= 40


# ---- 6. the executable ----
def test_rtow_radiance_at_direct_mis_prints_what_the_call_returns():
    scene_id, W, H, spp, depth, (i, j) = 7, 32, 24, 3, 6, (16, 12)   # the Cornell box: a quad lamp over diffuse walls
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    run = subprocess.run([exe, "--scene", str(scene_id), "--width", str(W), "--height", str(H), "--variant", "strict", "--spp", str(spp),
                          "--depth", str(depth), "--radiance-at", f"{i},{j}", "--direct", "mis"], check=True, cwd=ROOT, timeout=120,
                         capture_output=True, text=True)
    lines = [line for line in run.stdout.splitlines() if line.startswith("radiance ")]
    assert len(lines) == 1 and run.stdout.count("\n") == 1, run.stdout
    words = lines[0].split()
    assert words[1] == f"{i},{j}:" and [words[k] for k in (2, 4, 8, 10, 12, 14)] == ["samples", "radiance", "rays", "seconds", "shadow_rays", "reached"]
    scene = rt.builtin_scene(scene_id, 0, W, H)
    o, d, time0, _ = centre_rays(scene, W, H)
    k = j * W + i
    out, st = scene.radiance(o[k:k + 1].copy(), d[k:k + 1].copy(), time=time0, samples=spp, max_depth=depth, first_sequence=k,
                             want=("radiance", "path_rays"), stats=True, direct="mis", strategy=1)
    assert int(words[3]) == spp
    assert [float(x) for x in words[5:8]] == list(out["radiance"][0])
    assert int(words[9]) == out["path_rays"][0] and out["path_rays"][0] >= spp
    assert int(words[13]) == st.shadow_rays and int(words[15]) == st.shadow_reached and st.shadow_rays > 0
    assert float(words[11]) > 0.0, "the kernel's time"
    bad = subprocess.run([exe, "--scene", str(scene_id), "--radiance-at", f"{i},{j}", "--direct", "nee"], cwd=ROOT, timeout=120,
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "--direct" in bad.stderr
