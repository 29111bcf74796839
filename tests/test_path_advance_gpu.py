"""Path advances (rt_scene_path_advance, Scene.path_advance, PathBatch): one bounce for a batch of paths with the fold and the
compaction done on the device.  The keystone is the path step, which existing tests pin to the radiance query and through it to
the render: one advance is a path step, a mask and a fold restated in numpy, bit for bit and in order; fifty advances enqueued
without a wait in between are rt_scene_radiance bit for bit in the strict build.  Beside it the batch edges with guard rows, the
device count word, `alive`, carried throughputs and ids, the survivors' hit records, the fast build, repeatability and statistics.
Every ray set is at most 32 x 24 rays: three workgroups.
tests/test_path_advance_scale_gpu.py has the sizes beyond: up to 3137 workgroups, every level of the compaction's scan."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api
from query_helpers import bits
from test_path_step_gpu import STEP_SCENES, rays_of, scene_of, step_of
from test_radiance_gpu import EMITTED, SHELL_CENTRE, closed_form_sphere, shell_scene

pytestmark = pytest.mark.gpu

W, H = 32, 24
N = W * H
SEED = 1984
ALL = tuple(_lib.ADVANCE_OUTPUTS)
RAY = ("origin", "direction", "time", "rng_state", "throughput", "ray_id")
SCATTERED = 2
GUARDS = {"float64": 12345.678, "uint8": 0x5A, "uint32": 0x5A5A5A5A, "int32": 0x5A5A5A5A}
TORCH_TYPES = {"float64": torch.float64, "uint8": torch.uint8, "uint32": torch.int32, "int32": torch.int32}


# ---- the restatement: a path step, a mask and a fold ----
def expected(step, thr=None, ids=None, radiance=None, alive=None):
    """What include/rtow.h says an advance leaves, from the outputs of the path step of the same rays: (the survivors' rows by
    output name, the radiance array afterwards).  numpy float64, one operation at a time."""
    n = len(step["status"])
    thr = np.ones((n, 3)) if thr is None else thr
    ids = np.arange(n, dtype=np.int32) if ids is None else ids
    alive = np.ones(n, dtype=bool) if alive is None else alive != 0
    goes, ends = (step["status"] == SCATTERED) & alive, (step["status"] != SCATTERED) & alive
    out = {k: step[k][goes] for k in ("origin", "direction", "time", "rng_state", "t", "normal", "front_face", "material")}
    out["throughput"] = thr[goes] * step["attenuation"][goes]
    out["ray_id"] = ids[goes]
    after = None
    if radiance is not None:
        after = radiance.copy()
        for k in np.flatnonzero(ends):
            if 0 <= ids[k] < len(after):
                product = thr[k] * step["emitted"][k]
                after[ids[k]] = after[ids[k]] + product
    return out, after


def head(step, count):
    return {k: a[:count] for k, a in step.items()}


def same(got, want, keys=ALL):
    for k in keys:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    return True


def to_device(a):
    a = np.array(a)   # (a copy: the shared arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(name, tensor):
    a = tensor.cpu().numpy()
    return a.view(np.uint32) if name == "rng_state" else a


def device_inputs(name, **more):
    o, d, tm, states = rays_of(name)
    ins = {"origin": to_device(o), "direction": to_device(d), "time": to_device(tm), "rng_state": to_device(states)}
    ins.update({k: to_device(v) for k, v in more.items()})
    return ins


def guarded_outputs(rows, names=ALL):
    return {k: torch.full((rows,) + _lib.ADVANCE_OUTPUTS[k][1], GUARDS[_lib.ADVANCE_OUTPUTS[k][0]], dtype=TORCH_TYPES[_lib.ADVANCE_OUTPUTS[k][0]], device="cuda")
            for k in names}


def word(value):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


def workspace_for(capacity):
    nbytes = int(api.lib().rt_path_advance_workspace_bytes(capacity))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda"), nbytes


def raw(scene, capacity, ins, outs, radiance=None, count_in=None, count_out=None, variant=0, stats=None, first_sequence=0, workspace=None):
    """rt_scene_path_advance_device on torch tensors of the caller's, on the default stream; without `stats` it only enqueues.
    Returns the workspace, which the caller keeps until it has synchronized."""
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    ws, nbytes = workspace if workspace is not None else workspace_for(capacity)
    p = _lib.PathAdvanceParams(capacity, 0 if radiance is None else int(radiance.shape[0]), 0.0, SEED, first_sequence, variant, 0, None, ws.data_ptr(), nbytes)
    rays = _lib.PathAdvanceRays(*(ptr(ins.get(k)) for k in RAY + ("alive",)), ptr(count_in))
    out = _lib.PathAdvanceOut(ptr(radiance), *(ptr(outs.get(k)) for k in ALL), ptr(count_out))
    status = api.lib().rt_scene_path_advance_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), C.byref(stats) if stats is not None else None)
    assert status == 0, api.lib().rt_last_error().decode()
    return ws, nbytes


def survivors_of(outs, count, names=ALL):
    return {k: to_host(k, outs[k])[:count] for k in names}


@functools.lru_cache(maxsize=None)
def radiance_of(name, max_depth=50):
    o, d, tm, states = rays_of(name)
    return scene_of(name).radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=max_depth, variant=0)["radiance"]


# ---- 1. one advance is a path step and a mask ----
@pytest.mark.parametrize("name", ["mixed bvh", "mixed list", "scene 9 list", "scene 7 bvh"])
def test_one_advance_is_a_path_step_a_mask_and_a_fold(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    want, want_radiance = expected(step_of(name), radiance=np.zeros((N, 3)))
    survivors = len(want["ray_id"])
    assert 0 < survivors < N, "some paths end and some go on"
    # the host call
    radiance = np.zeros((N, 3))
    got = scene.path_advance(o, d, times=tm, rng_state=states, radiance=radiance, want=ALL)
    assert len(got["ray_id"]) == survivors and same(got, want)
    assert np.array_equal(bits(radiance), bits(want_radiance)), "0 + thr * emitted for the ended ids, the others untouched"
    assert (np.diff(got["ray_id"]) > 0).all(), "input order is kept"
    # the device call
    ins = device_inputs(name)
    kept = {k: t.clone() for k, t in ins.items()}
    dev_radiance = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    got = scene.path_advance(ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"], radiance=dev_radiance, want=ALL)
    for k, a in got.items():
        assert isinstance(a, torch.Tensor) and a.is_cuda and a.shape[0] == survivors, k
    assert same({k: to_host(k, a) for k, a in got.items()}, want)
    assert np.array_equal(bits(dev_radiance.cpu().numpy()), bits(want_radiance))
    for k in ins:
        assert torch.equal(ins[k], kept[k]), "the inputs are only read"


# ---- 2. edges ----
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 513, 768])
def test_batch_edges_write_exactly_their_rows(count):
    for name in ("mixed bvh", "mixed list"):
        scene = scene_of(name)
        ins = device_inputs(name)   # longer than count: only count rows are read
        want, want_radiance = expected(head(step_of(name), count), radiance=np.zeros((count, 3)))
        outs = guarded_outputs(count + 1)
        radiance = torch.cat([torch.zeros((count, 3), dtype=torch.float64), torch.full((1, 3), GUARDS["float64"], dtype=torch.float64)]).cuda()
        live = torch.full((2,), GUARDS["int32"], dtype=torch.int32, device="cuda")
        keep = raw(scene, count, ins, outs, radiance=radiance[:count], count_out=live)
        torch.cuda.synchronize()
        del keep
        survivors = int(live[0])
        assert survivors == len(want["ray_id"]) and int(live[1]) == GUARDS["int32"], name
        assert same(survivors_of(outs, survivors), want), name
        for k, (dtype, _) in _lib.ADVANCE_OUTPUTS.items():
            got = outs[k].cpu().numpy()
            assert (got[count] == np.array(GUARDS[dtype]).astype(got.dtype)).all(), f"{name}: {k}: the row behind the capacity was written"
        got = radiance.cpu().numpy()
        assert np.array_equal(bits(got[:count]), bits(want_radiance)) and (got[count] == GUARDS["float64"]).all(), name


def _starts(gen):
    return SHELL_CENTRE + gen.integers(-36, 37, size=(N, 3)) / 64.0


@pytest.mark.parametrize("world", ["bvh", "list"])
def test_all_none_and_misses(world):
    """Three extreme batches: every ray survives (towards a perfect mirror), none does (inside an emissive shell), every ray misses."""
    gen = np.random.default_rng(6)
    start = np.ascontiguousarray(_starts(gen))
    target = SHELL_CENTRE + np.concatenate([gen.integers(-96, 97, size=(N, 2)) / 64.0, np.full((N, 1), -5.0)], axis=1)
    mirror = shell_scene(world, mirror=True)
    d = np.ascontiguousarray(target - start)
    radiance = np.zeros((N, 3))
    got = mirror.path_advance(start, d, radiance=radiance, want=ALL)
    step = mirror.path_step(start, d, want=tuple(_lib.STEP_OUTPUTS))
    assert len(got["ray_id"]) == N and (step["status"] == SCATTERED).all() and same(got, expected(step)[0])
    assert np.array_equal(got["ray_id"], np.arange(N)) and (radiance == 0).all()
    d = np.ascontiguousarray(gen.normal(size=(N, 3)))
    radiance = np.zeros((N, 3))
    got = shell_scene(world).path_advance(start, d, radiance=radiance, want=ALL)
    assert all(len(got[k]) == 0 for k in ALL) and (radiance == EMITTED).all()
    s, o, d, bg, _, hits = closed_form_sphere()
    o, d = np.ascontiguousarray(o[~hits]), np.ascontiguousarray(d[~hits])
    radiance = np.zeros((len(o), 3))
    got = s.path_advance(o, d, radiance=radiance, want=ALL)
    assert all(len(got[k]) == 0 for k in ALL) and (radiance == bg).all()


# ---- 3. the fold is the radiance ----
def enqueue_fold(scene, name, bounces):
    """`bounces` advances between two sets of arrays through one count word, enqueued without a wait; returns the radiance tensor,
    the count word and what has to stay allocated."""
    sides = [device_inputs(name, throughput=np.ones((N, 3)), ray_id=np.arange(N, dtype=np.int32)), guarded_outputs(N, RAY)]
    radiance = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
    live = word(N)
    workspace = workspace_for(N)
    for k in range(bounces):
        raw(scene, N, sides[k % 2], sides[1 - k % 2], radiance=radiance, count_in=live, count_out=live, workspace=workspace)
    return radiance, live, (sides, workspace)


@pytest.mark.parametrize("name", sorted(STEP_SCENES))
def test_fifty_advances_enqueued_at_once_are_the_radiance_bit_for_bit(name):
    scene = scene_of(name)
    want = radiance_of(name)
    torch.cuda.synchronize()
    radiance, live, keep = enqueue_fold(scene, name, 50)
    torch.cuda.synchronize()   # the one wait
    got = radiance.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), f"{np.sum((bits(got) != bits(want)).any(axis=-1))} of {N} rays differ"
    print(f"{name}: {int(live[0])} rays alive after 50 bounces")


@pytest.mark.parametrize("check_every", [0, 1, 8])
@pytest.mark.parametrize("name", sorted(STEP_SCENES))
def test_path_batch_run_is_the_radiance_bit_for_bit(name, check_every):
    ins = device_inputs(name)
    batch = rt.PathBatch(scene_of(name), ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"])
    got = batch.run(50, check_every=check_every)
    torch.cuda.synchronize()
    assert got is batch.radiance and np.array_equal(bits(got.cpu().numpy()), bits(radiance_of(name)))


def test_offsets_across_workgroups_are_exercised_for_several_bounces():
    """The closed box of scene 7: more than a workgroup's worth of rays is still alive after three advances, in all three
    workgroups' ranges, and the batch's rows are the host fold's."""
    name = "scene 7 bvh"
    ins = device_inputs(name)
    batch = rt.PathBatch(scene_of(name), ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"], hits=True)
    step, thr, ids = step_of(name), None, None
    scene = scene_of(name)
    for bounce in range(3):
        batch.advance()
        want, _ = expected(step, thr=thr, ids=ids)
        live = batch.live()
        assert live == len(want["ray_id"])
        assert same({k: to_host(k, getattr(batch, k))[:live] for k in ALL}, want), bounce
        thr, ids = want["throughput"], want["ray_id"]
        step = scene.path_step(want["origin"], want["direction"], times=want["time"], rng_state=want["rng_state"], want=tuple(_lib.STEP_OUTPUTS))
    print(f"{name}: {live} rays alive after the third advance")
    assert live > 256


def test_a_depth_cut_drops_the_rays_still_alive():
    name = "mixed list"
    ins = device_inputs(name)
    batch = rt.PathBatch(scene_of(name), ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"])
    got = batch.run(4, check_every=0)
    assert batch.live() > 0, "some path is cut at max_depth"
    assert np.array_equal(bits(got.cpu().numpy()), bits(radiance_of(name, 4)))
    assert not np.array_equal(bits(radiance_of(name, 4)), bits(radiance_of(name)))


def test_a_throughput_scaled_in_place_scales_the_radiance():
    """What Russian roulette does to a winner: the attribute is the tensor the next advance reads.  A power of two scales every
    product and every sum exactly."""
    name = "mixed bvh"
    ins = device_inputs(name)
    batch = rt.PathBatch(scene_of(name), ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"])
    batch.throughput.mul_(0.5)
    assert np.array_equal(bits(batch.run(50).cpu().numpy()), bits(0.5 * radiance_of(name)))


def test_path_batch_seeds_as_the_radiance_query_does():
    name = "mixed bvh"
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    want = scene.radiance(o, d, times=tm, seed=7, first_sequence=5, samples=1, max_depth=50)["radiance"]
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), seed=7, first_sequence=5)
    assert np.array_equal(bits(batch.run(50).cpu().numpy()), bits(want))


# ---- 4. the device count word ----
def test_the_count_word_limits_the_rows_and_is_clamped_to_the_capacity():
    name = "mixed bvh"
    scene = scene_of(name)
    ins = device_inputs(name)
    for said, rows in ((300, 300), (900, N), (0, 0)):
        want, want_radiance = expected(head(step_of(name), rows), radiance=np.zeros((N, 3)))
        outs = guarded_outputs(N + 1)
        radiance = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
        given, live = word(said), word(-1)
        keep = raw(scene, N, ins, outs, radiance=radiance, count_in=given, count_out=live)
        torch.cuda.synchronize()
        del keep
        assert int(given[0]) == said and int(live[0]) == len(want["ray_id"])
        assert same(survivors_of(outs, int(live[0])), want), said
        assert np.array_equal(bits(radiance.cpu().numpy()), bits(want_radiance)), "rows at and beyond the word are not stepped"
        for k, (dtype, _) in _lib.ADVANCE_OUTPUTS.items():
            got = outs[k].cpu().numpy()
            assert (got[N] == np.array(GUARDS[dtype]).astype(got.dtype)).all(), k


def test_one_word_is_input_and_output_of_two_chained_calls():
    name = "scene 7 bvh"
    scene = scene_of(name)
    first, _ = expected(step_of(name))
    second_step = scene.path_step(first["origin"], first["direction"], times=first["time"], rng_state=first["rng_state"], want=tuple(_lib.STEP_OUTPUTS))
    second, _ = expected(second_step, thr=first["throughput"], ids=first["ray_id"])
    ins = device_inputs(name)
    middle, last = guarded_outputs(N, RAY), guarded_outputs(N)
    live = word(N)
    keep = [raw(scene, N, ins, middle, count_in=live, count_out=live), raw(scene, N, middle, last, count_in=live, count_out=live)]
    torch.cuda.synchronize()
    del keep
    assert int(live[0]) == len(second["ray_id"]) < len(first["ray_id"])
    assert same(survivors_of(last, int(live[0])), second)


# ---- 5. alive ----
def test_dead_rays_are_dropped_untraced():
    name = "mixed list"
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    alive = np.ones(N, dtype=np.uint8)
    alive[::3] = 0
    want, want_radiance = expected(step_of(name), radiance=np.full((N, 3), 0.25), alive=alive)
    radiance = np.full((N, 3), 0.25)
    got = scene.path_advance(o, d, times=tm, rng_state=states, alive=alive, radiance=radiance, want=ALL)
    assert same(got, want) and np.array_equal(bits(radiance), bits(want_radiance))
    assert (radiance[::3] == 0.25).all() and not np.isin(got["ray_id"], np.arange(N)[::3]).any()
    kept = alive != 0   # the call on the kept rays alone (the ids say which)
    alone = scene.path_advance(*(np.ascontiguousarray(a[kept]) for a in (o, d)), times=np.ascontiguousarray(tm[kept]),
                               rng_state=np.ascontiguousarray(states[kept]), ray_id=np.arange(N, dtype=np.int32)[kept].copy(), want=ALL)
    assert same(alone, got)
    ins = device_inputs(name)   # and through PathBatch.kill
    batch = rt.PathBatch(scene, ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"])
    batch.kill(to_device(alive) == 0)
    batch.advance()
    live = batch.live()
    assert same({k: to_host(k, getattr(batch, k))[:live] for k in RAY}, want, RAY)
    assert bool((batch._alive == 1).all()), "the marks are forgotten after the advance"


# ---- 6. carried state ----
def test_throughputs_and_ids_are_carried_and_the_radiance_lands_at_the_ids_row():
    name = "mixed bvh"
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    gen = np.random.default_rng(11)
    thr = np.ascontiguousarray(gen.uniform(0.05, 1.5, (N, 3)))
    ids = gen.permutation(N).astype(np.int32) - 20   # twenty below the range, and with sources = N - 60 forty beyond it
    sources = N - 60
    start = np.ascontiguousarray(gen.uniform(0.0, 2.0, (sources, 3)))
    want, want_radiance = expected(step_of(name), thr=thr, ids=ids, radiance=start)
    for device in (False, True):
        args = [o, d, tm, states, thr, ids, start.copy()]
        if device:
            args = [to_device(a) for a in args]
        got = scene.path_advance(args[0], args[1], times=args[2], rng_state=args[3], throughput=args[4], ray_id=args[5], radiance=args[6], want=ALL)
        if device:
            got, args[6] = {k: to_host(k, a) for k, a in got.items()}, args[6].cpu().numpy()
        assert same(got, want), device
        assert np.array_equal(bits(args[6]), bits(want_radiance)), "rounded product, then the sum, at the id's row"
    ended = ids[step_of(name)["status"] != SCATTERED]
    assert (ended < 0).any() and (ended >= sources).any(), "ids on both sides of the range ended, and added nothing"
    assert not np.array_equal(want_radiance, start)


# ---- 7. the hit record of the survivors ----
@pytest.mark.parametrize("name", ["mixed bvh", "mixed list", "scene 7 bvh", "scene 12 bvh"])
def test_the_survivors_hit_record_is_the_ray_querys(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    record = ("t", "normal", "front_face", "material")
    got = scene.path_advance(o, d, times=tm, rng_state=states, want=("ray_id",) + record)
    query = scene.intersect(o, d, times=tm, want=record)
    assert len(got["ray_id"]) > 0
    for key in record:
        assert np.array_equal(bits(got[key]), bits(query[key][got["ray_id"]])), key
    assert np.isfinite(got["t"]).all() and (got["material"] != 255).all()


# ---- 8. the fast build ----
@pytest.mark.parametrize("name", ["mixed bvh", "scene 9 list"])
def test_the_fast_build_keeps_the_fast_steps_rows(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    gen = np.random.default_rng(12)
    thr = np.ascontiguousarray(gen.uniform(0.05, 1.5, (N, 3)))
    want, want_radiance = expected(step_of(name, 1), thr=thr, radiance=np.zeros((N, 3)))
    radiance = np.zeros((N, 3))
    got = scene.path_advance(o, d, times=tm, rng_state=states, throughput=thr, radiance=radiance, variant=1, want=ALL)
    assert same(got, want), "thr * attenuation is one multiply"
    assert np.array_equal(bits(radiance), bits(want_radiance)), "0 + thr * emitted is exact, fused or not"


# ---- 9. repeatability and neighbours ----
def test_the_same_call_twice_and_a_film_before_and_after():
    name = "scene 7 bvh"
    scene = scene_of(name)
    film = rt.Film(W, H)
    before_stats = film.render(scene, 2, variant=0)
    before = film.download()
    ins = device_inputs(name)
    runs = []
    for _ in range(2):
        radiance = torch.zeros((N, 3), dtype=torch.float64, device="cuda")
        got = scene.path_advance(ins["origin"], ins["direction"], times=ins["time"], rng_state=ins["rng_state"], radiance=radiance, want=ALL)
        runs.append(dict({k: to_host(k, a) for k, a in got.items()}, radiance=radiance.cpu().numpy()))
    assert same(runs[0], runs[1], ALL + ("radiance",))
    after_stats = film.render(scene, 2, variant=0)
    assert np.array_equal(bits(film.download()), bits(before)), "the same frame before and after the advances"
    assert (before_stats.rays, before_stats.samples, before_stats.kernel_kind, before_stats.lds_bytes) == \
        (after_stats.rays, after_stats.samples, after_stats.kernel_kind, after_stats.lds_bytes)


def test_a_scene_destroyed_behind_enqueued_advances_waits_for_them():
    """rt_scene_destroy waits for the last advance enqueued: the radiance of a scene that is gone by the time it is read."""
    name = "mixed bvh"
    scene = STEP_SCENES[name]()   # one of this test's own
    radiance, live, keep = enqueue_fold(scene, name, 50)
    del scene
    torch.cuda.synchronize()
    assert np.array_equal(bits(radiance.cpu().numpy()), bits(radiance_of(name)))


# ---- 10. statistics ----
@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_statistics_count_the_rays_and_leave_the_outputs_alone(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    o, d, tm, states = (np.ascontiguousarray(a[:100]) for a in (o, d, tm, states))   # one full wave and a ragged one
    alive = np.ones(100, dtype=np.uint8)
    alive[5] = alive[70] = 0
    plain = scene.path_advance(o, d, times=tm, rng_state=states, alive=alive, want=ALL)
    counted, st = scene.path_advance(o, d, times=tm, rng_state=states, alive=alive, want=ALL, stats=True)
    print(f"{name}: {st.scattered} of {st.rays} rays scattered, {st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch, {st.seconds * 1e3:.3f} ms")
    assert same(counted, plain)
    assert st.rays == 98 and st.scattered == len(plain["ray_id"]) > 0
    assert st.kernel_vgprs > 0 and st.seconds > 0
    ins = {"origin": to_device(o), "direction": to_device(d), "time": to_device(tm), "rng_state": to_device(states)}
    outs, live, st = guarded_outputs(100), word(-1), _lib.PathAdvanceStats()
    raw(scene, 100, ins, outs, count_in=word(64), count_out=live, stats=st)   # with statistics the device call waits
    assert st.rays == 64 and st.scattered == int(live[0]) > 0
