"""Path advances at the sizes README and DESIGN quote them for: the compaction (csrc/advance_pack.hip) beyond the three workgroups
of tests/test_path_advance_gpu.py -- the exchange between the sixteen waves of the scan workgroup (more than 64 workgroup counts,
16 384 rows), the carry across the trips of its loop (more than 1024 counts, 262 144 rows), the offsets of every workgroup of the
gathers, and a count word far above 768 handed from one call to the next.  Every comparison is bit for bit, against a closed form
(towards a perfect mirror every stepped ray scatters, so the survivors are np.flatnonzero(alive) and their number alive.sum()) or
against a call the suite already pins: the path step, the radiance query, the restatement of the advance with light samples.
tests/advance_scale_masks.py has the sizes and the masks; tests/test_path_advance_scale_host.py checks without a GPU that they
reach every level of the scan.  The rays are a few hundred tiled with np.tile and, but for the light samples, seeded by position,
so one path step of the longest set is the reference of every size: a shorter set is its head."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api
import test_path_advance_direct_gpu as direct
from advance_scale_masks import LARGEST, MASKS, ROWS, SIZES, alive_of
from query_helpers import bits
from test_path_advance_gpu import ALL, GUARDS, RAY, SCATTERED, SEED, expected, guarded_outputs, head, raw, same, to_host, word, workspace_for
from test_path_step_gpu import rays_of, scene_of
from test_radiance_gpu import SHELL_CENTRE, shell_scene

pytestmark = pytest.mark.gpu

STEP_ALL = tuple(_lib.STEP_OUTPUTS)
BASE = 768


def tiled(a, rows):
    """Row k is a[k % len(a)]: the head of a longer tiling is the shorter one."""
    a = np.asarray(a)
    return np.ascontiguousarray(np.tile(a, (-(-rows // len(a)),) + (1,) * (a.ndim - 1))[:rows])


def frozen(arrays):
    for a in (arrays.values() if isinstance(arrays, dict) else arrays):
        a.setflags(write=False)
    return arrays


def on_device(a):
    a = np.array(a)   # (a copy: the shared arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


# ---- the world with a closed form: every ray is on its way to a perfect mirror ----
def mirror():
    return shell_scene("bvh", mirror=True)


@functools.lru_cache(maxsize=None)
def mirror_rays():
    """The rays of test_all_none_and_misses' first batch, tiled to the longest size."""
    gen = np.random.default_rng(6)
    start = SHELL_CENTRE + gen.integers(-36, 37, size=(BASE, 3)) / 64.0
    target = SHELL_CENTRE + np.concatenate([gen.integers(-96, 97, size=(BASE, 2)) / 64.0, np.full((BASE, 1), -5.0)], axis=1)
    return frozen((tiled(start, LARGEST), tiled(target - start, LARGEST)))


@functools.lru_cache(maxsize=None)
def mirror_step():
    """The path step of the longest set, seeded by position: computed once, shared, and its head is the step of every size."""
    o, d = mirror_rays()
    step = mirror().path_step(o, d, seed=SEED, first_sequence=0, want=STEP_ALL)
    assert (step["status"] == SCATTERED).all(), "the mask alone decides who survives"
    assert not np.array_equal(step["rng_state"][0], step["rng_state"][BASE]), "equal rays, but a stream each"
    return frozen(step)


@functools.lru_cache(maxsize=None)
def mirror_inputs():
    o, d = mirror_rays()
    return {"origin": on_device(o), "direction": on_device(d)}


def advance(scene, rows, ins, alive=None, count_in=None, workspace=None, call=raw, sources=None, **more):
    """One raw device call of capacity `rows` into outputs of rows + 1 guard rows, a zeroed radiance array and a guarded pair of
    count words.  Returns (the count, the survivors' rows on the host, the radiance on the host); asserts what must hold of every
    call: the count is at most the capacity, and the row behind the capacity and the word behind the count keep their guards."""
    names = tuple(more.pop("names", ALL))
    outs = guarded_outputs(rows + 1, [k for k in names if k in _lib.ADVANCE_OUTPUTS])
    if "scatter_pdf" in names:
        outs["scatter_pdf"] = torch.full((rows + 1,), GUARDS["float64"], dtype=torch.float64, device="cuda")
    ins = dict(ins)
    if alive is not None:
        ins["alive"] = on_device(alive)
    radiance = torch.zeros((rows if sources is None else sources, 3), dtype=torch.float64, device="cuda")
    live = torch.full((2,), GUARDS["int32"], dtype=torch.int32, device="cuda")
    given = None if count_in is None else word(count_in)
    keep = call(scene, rows, ins, outs, radiance=radiance, count_in=given, count_out=live, workspace=workspace, **more)
    torch.cuda.synchronize()
    del keep
    count = int(live[0])
    assert 0 <= count <= rows and int(live[1]) == GUARDS["int32"], "the word behind the count was written"
    for k in names:
        behind = outs[k][rows].cpu().numpy()
        assert (behind == np.array(GUARDS["float64" if k == "scatter_pdf" else _lib.ADVANCE_OUTPUTS[k][0]]).astype(behind.dtype)).all(), \
            f"{k}: the row behind the capacity was written"
    if given is not None:
        assert int(given[0]) == count_in, "the count that came in is only read"
    return count, {k: to_host(k, outs[k][:count]) for k in names}, radiance.cpu().numpy()


# ---- 1. sizes x masks ----
@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("size", list(SIZES))
def test_the_survivors_are_the_alive_rows_in_order(size, mask):
    """Every size of the scan (workgroup counts 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 65) under every mask.  The packed ids
    are np.flatnonzero(alive) and the count is alive.sum() -- neither needs the library to state -- and every output row is the
    path step's, masked and folded by `expected`.
    Guards: include/rtow.h says "Output rows from the survivors' count up to params->count are unspecified", so of the rows the
    call must not touch only the one at the capacity can be asserted, and it is, in every output, with the word behind count_out."""
    rows = SIZES[size]
    alive = alive_of(mask, rows)
    started = time.perf_counter()
    count, got, radiance = advance(mirror(), rows, mirror_inputs(), alive=alive)
    called = time.perf_counter()
    assert count == int(alive.sum())
    assert np.array_equal(got["ray_id"], np.flatnonzero(alive))
    want, _ = expected(head(mirror_step(), rows), alive=alive)
    assert same(got, want)
    assert not radiance.any(), "nobody ended"
    print(f"{size} workgroups, {mask}: {count} of {rows} rows survive; the call and its copies {called - started:.3f} s, the comparison {time.perf_counter() - called:.3f} s")


# ---- 2. the count word that comes in ----
@pytest.mark.parametrize("said", [16385, 262145, SIZES["1025"] + 7])
def test_a_count_word_of_many_workgroups_limits_the_rows(said):
    """A *count_in of 65 and of 1025 workgroups' rows (one row in the last), and one beyond the capacity, which is clamped: with
    every row alive the survivors are exactly the rows below min(*count_in, capacity)."""
    rows = SIZES["1025"]
    stepped = min(said, rows)
    count, got, radiance = advance(mirror(), rows, mirror_inputs(), alive=alive_of("all", rows), count_in=said)
    assert count == stepped
    assert np.array_equal(got["ray_id"], np.arange(stepped))
    assert same(got, expected(head(mirror_step(), stepped))[0])
    assert not radiance.any()


# ---- 3. the world decides who scatters ----
@functools.lru_cache(maxsize=None)
def world_rays(name):
    o, d, tm, _ = rays_of(name)
    rows = SIZES["1025"]   # (761 of the 768, a prime: no two workgroups of a size hold the same rays)
    return frozen((tiled(o[:761], rows), tiled(d[:761], rows), tiled(tm[:761], rows)))


@functools.lru_cache(maxsize=None)
def world_step(name):
    o, d, tm = world_rays(name)
    return frozen(scene_of(name).path_step(o, d, times=tm, seed=SEED, first_sequence=0, want=STEP_ALL))


@pytest.mark.parametrize("size", ["65", "1025"])
@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_survivors_the_world_chooses(name, size):
    """The camera rays of the mixed worlds, tiled and seeded by position: misses, lamps and absorbing metal end some paths in every
    workgroup, so the workgroup counts are whatever the world gives.  The radiance of the ended rows is restated here without
    `expected`'s loop: fresh rays carry (1, 1, 1) and distinct ids, so row k ends with 0 + (1, 1, 1) * emitted."""
    rows = SIZES[size]
    o, d, tm = world_rays(name)
    ins = {"origin": on_device(o[:rows]), "direction": on_device(d[:rows]), "time": on_device(tm[:rows])}
    step = head(world_step(name), rows)
    want, _ = expected(step)
    count, got, radiance = advance(scene_of(name), rows, ins)
    assert count == len(want["ray_id"]) and 0 < count < rows, "some paths end and some go on"
    assert same(got, want)
    ended = step["status"] != SCATTERED
    want_radiance = np.zeros((rows, 3))
    product = np.ones((int(ended.sum()), 3)) * step["emitted"][ended]
    want_radiance[ended] = want_radiance[ended] + product
    assert np.array_equal(bits(radiance), bits(want_radiance))
    per_workgroup = np.add.reduceat((step["status"] == SCATTERED).astype(np.int64), np.arange(0, rows, ROWS))
    assert len(set(per_workgroup.tolist())) > 8, "many different workgroup counts"


# ---- 4. chains through one count word ----
CHAIN = 262145   # 1025 workgroups, one row in the last


@functools.lru_cache(maxsize=None)
def box_rays():
    o, d, tm, _ = rays_of("scene 7 bvh")
    return frozen((tiled(o, CHAIN), tiled(d, CHAIN), tiled(tm, CHAIN)))


def box_batch(**kw):
    o, d, tm = box_rays()
    return rt.PathBatch(scene_of("scene 7 bvh"), on_device(o), on_device(d), times=on_device(tm), seed=SEED, first_sequence=0, **kw)


@pytest.mark.parametrize("check_every", [8, 0])
def test_a_path_batch_of_1025_workgroups_runs_to_the_radiance_bit_for_bit(check_every):
    """The closed box of scene 7 keeps its rays alive: fifty advances through one count word that starts at 262 145, against
    Scene.radiance of the same rays -- with the count read every eight bounces (PathBatch.run's default) and never.
    Only the first advance has more than 1024 workgroup counts, and its last workgroup holds one ray: the chains are about the
    count word and the waves of the scan; the carry between its trips is what the sizes and masks above are for."""
    want = box_radiance()
    got = box_batch().run(50, check_every=check_every)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), f"{np.sum((bits(got) != bits(want)).any(axis=-1))} of {CHAIN} rays differ"


@functools.lru_cache(maxsize=None)
def box_radiance():
    o, d, tm = box_rays()
    return scene_of("scene 7 bvh").radiance(o, d, times=tm, seed=SEED, first_sequence=0, samples=1, max_depth=50, variant=0)["radiance"]


def test_three_advances_of_1025_workgroups_are_the_host_fold():
    """test_offsets_across_workgroups_are_exercised_for_several_bounces at 262 145 rays: after each of three advances the batch's
    rows, hit records included, are the host fold's, and the count that the next advance reads still spans several waves of the
    scan workgroup."""
    scene = scene_of("scene 7 bvh")
    o, d, tm = box_rays()
    batch = box_batch(hits=True)
    step = scene.path_step(o, d, times=tm, seed=SEED, first_sequence=0, want=STEP_ALL)
    thr, ids = None, None
    for bounce in range(3):
        batch.advance()
        want, _ = expected(step, thr=thr, ids=ids)
        live = batch.live()
        assert live == len(want["ray_id"]), bounce
        assert same({k: to_host(k, getattr(batch, k))[:live] for k in ALL}, want), bounce
        thr, ids = want["throughput"], want["ray_id"]
        if bounce < 2:
            step = scene.path_step(want["origin"], want["direction"], times=want["time"], rng_state=want["rng_state"], want=STEP_ALL)
    print(f"scene 7 bvh: {live} of {CHAIN} rays alive after the third advance")
    assert live > 16384, "the chained count word spans several waves of the scan"


# ---- 5. a workspace used before ----
@pytest.mark.parametrize("rows", [513, 512 * ROWS + 1], ids=["513 rows", "513 workgroups"])
def test_a_workspace_left_by_a_larger_call_changes_nothing(rows):
    """include/rtow.h leaves the workspace's layout private; csrc says the two launches behind the step "read nothing stale".  A
    workspace of 2049 workgroups is filled by a call in which every workgroup counts its full rows; a smaller call on it, with half
    of its rows alive, then gives what it gives on a workspace of its own, which is the closed form."""
    large = SIZES["2049"]
    workspace = workspace_for(large)
    count, _, _ = advance(mirror(), large, mirror_inputs(), workspace=workspace, names=("origin", "direction", "ray_id"))
    assert count == large
    alive = alive_of("half", rows)
    used = advance(mirror(), rows, mirror_inputs(), alive=alive, workspace=workspace)
    fresh = advance(mirror(), rows, mirror_inputs(), alive=alive)
    assert used[0] == fresh[0] == int(alive.sum())
    assert same(used[1], fresh[1]) and np.array_equal(used[1]["ray_id"], np.flatnonzero(alive))
    assert same(used[1], expected(head(mirror_step(), rows), alive=alive)[0])


# ---- 6. another stream; light samples ----
def call_on(scene, capacity, ins, outs, radiance=None, count_in=None, count_out=None, workspace=None, stream=None, light=None):
    """The raw device call with what test_path_advance_gpu.raw leaves at its default: the stream of the params, and with
    `light` = (strategy, sample) the call with light samples, rt_scene_path_advance_direct_device.  Only enqueues."""
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    bytes_of = api.lib().rt_path_advance_direct_workspace_bytes if light else api.lib().rt_path_advance_workspace_bytes
    nbytes = int(bytes_of(capacity))
    ws = workspace[0] if workspace is not None else torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    params = (capacity, 0 if radiance is None else int(radiance.shape[0]), 0.0, SEED, 0, 0, 0, stream, ws.data_ptr(), nbytes)
    ray_arrays = tuple(ptr(ins.get(k)) for k in RAY + ("alive",)) + (ptr(count_in),)
    out_arrays = (ptr(radiance),) + tuple(ptr(outs.get(k)) for k in _lib.ADVANCE_OUTPUTS) + (ptr(count_out),)
    if light:
        p = _lib.PathAdvanceDirectParams(*params, (C.c_int32 * 4)(), light[0], light[1])
        rays = _lib.PathAdvanceDirectRays(*ray_arrays, ptr(ins.get("scatter_pdf")))
        out = _lib.PathAdvanceDirectOut(*out_arrays, ptr(outs.get("scatter_pdf")))
        status = api.lib().rt_scene_path_advance_direct_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    else:
        p, rays, out = _lib.PathAdvanceParams(*params), _lib.PathAdvanceRays(*ray_arrays), _lib.PathAdvanceOut(*out_arrays)
        status = api.lib().rt_scene_path_advance_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    assert status == 0, api.lib().rt_last_error().decode()
    return ws


def test_a_side_stream_gives_the_same_bits():
    """The 1025-workgroup set with half of its rows alive, enqueued on a stream other than the default: all three launches of the
    call go to the stream of the params.  (`advance` fills inputs and guards on the default stream and waits before the call.)"""
    rows = SIZES["1025"]
    alive = alive_of("half", rows)
    plain = advance(mirror(), rows, mirror_inputs(), alive=alive)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream

    def on_side(*args, **kw):
        torch.cuda.synchronize()
        keep = call_on(*args, stream=side.cuda_stream, **kw)
        side.synchronize()
        return keep

    other = advance(mirror(), rows, mirror_inputs(), alive=alive, call=on_side)
    assert other[0] == plain[0] == int(alive.sum())
    assert same(other[1], plain[1]) and np.array_equal(other[1]["ray_id"], np.flatnonzero(alive))
    assert not other[2].any()


LIGHT_ALL = tuple(_lib.ADVANCE_DIRECT_OUTPUTS)


@functools.lru_cache(maxsize=None)
def lamp_rays():
    """The thousand rays of the light-sample tests, streams and carried densities included, tiled to 1025 workgroups; fresh
    throughputs and an id a row."""
    base, rows = direct.rays(), SIZES["1025"]
    live = {k: tiled(base[k], rows) for k in ("origin", "direction", "time", "rng_state", "scatter_pdf")}
    live.update(throughput=np.ones((rows, 3)), ray_id=np.arange(rows, dtype=np.int32))
    return frozen(live)


@pytest.mark.parametrize("mask", ["half", "one a workgroup"])
@pytest.mark.parametrize("size", ["65", "1025"])
def test_light_samples_at_many_workgroups_are_the_restatement(size, mask):
    """rt_scene_path_advance_direct_device, one bounce of strategy 1 with light samples on the lamp scene, against
    test_path_advance_direct_gpu.restated: the survivors' rows with the density they were sent with (the one array the second
    gather moves and the first does not), the radiance after the light samples and the weighted lamps, and the count.
    The lamp scene ends some alive rays (misses and lamps), so the ids are the restatement's and not np.flatnonzero(alive); they
    are a part of it, in order."""
    rows = SIZES[size]
    scene = direct.world("lamp scene")
    live = {k: np.ascontiguousarray(a[:rows]) for k, a in lamp_rays().items()}
    alive = alive_of(mask, rows)
    want, want_radiance, told = direct.restated(scene, live, np.zeros((rows, 3)), 1, True, alive)
    ins = {k: on_device(a) for k, a in live.items()}
    count, got, radiance = advance(scene, rows, ins, alive=alive, call=call_on, light=(1, 1), names=LIGHT_ALL)
    assert count == len(want["ray_id"]) and 0 < count < int(alive.sum()), "some alive rays end and some go on"
    assert direct.same(got, want, LIGHT_ALL)
    assert np.array_equal(bits(radiance), bits(want_radiance))
    assert np.isin(got["ray_id"], np.flatnonzero(alive)).all() and (np.diff(got["ray_id"]) > 0).all()
    assert told["cast"] > 0 and (got["scatter_pdf"] > 0).any(), "light samples were taken"
    assert not radiance[alive == 0].any(), "a dead row adds nothing"
