"""The two calls of every ray-batch family -- ray queries, radiance, radiance with light samples, path steps, light samples, light
densities and both path advances -- against each other: the call on host arrays stages them, runs the call on device arrays and
copies the results back, so for the same rays both give the same bits, with statistics and without.  Beside it what only the host
call does: an occlusion query leaves the outputs it does not write alone, and the advances read rays->count from a host word.
One world ("mixed bvh": every primitive, texture and material kind, one lamp) and 100 of its camera rays: a full wave and a ragged
one."""
import ctypes as C

import numpy as np
import pytest
import torch

from raytracinginoneweekendincuda_amd import _lib, api
from query_helpers import bits
from test_path_step_gpu import rays_of, scene_of, step_of

pytestmark = pytest.mark.gpu

NAME = "mixed bvh"
ROWS = 100
SEED = 1984
GUARDS = {"float64": 12345.678, "uint8": 0x5A, "uint32": 0x5A5A5A5A, "int32": 0x5A5A5A5A}
RAY = ("origin", "direction", "time", "rng_state", "throughput", "ray_id")
PLAIN = tuple(_lib.ADVANCE_OUTPUTS)


def to_device(a):
    a = np.array(a)   # (a copy: the shared arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(a, like):
    a = a.cpu().numpy()
    return a.view(np.uint32) if like.dtype == np.uint32 else a


def batch(rows=ROWS):
    """`rows` camera rays from all over the frame (sky, floor and every object: some paths end, some go on) with their streams, and
    what the advances and the light calls take beside them: throughputs, ids (one outside the radiance array), one dead ray,
    densities, and the points the first step scattered to.  Fresh copies."""
    every = len(rays_of(NAME)[0]) // rows
    o, d, tm, states = (np.array(a[::every][:rows]) for a in rays_of(NAME))
    step = {k: np.array(a[::every][:rows]) for k, a in step_of(NAME).items()}
    gen = np.random.default_rng(7)
    ids = np.arange(rows, dtype=np.int32)
    ids[5] = rows + 7
    alive = np.ones(rows, dtype=np.uint8)
    alive[3] = 0
    return dict(origin=o, direction=d, time=tm, rng_state=states, throughput=np.ascontiguousarray(gen.uniform(0.25, 1.0, (rows, 3))), ray_id=ids,
                alive=alive, scatter_pdf=np.where(np.arange(rows) % 3 == 1, 0.25, 0.0), radiance=np.full((rows, 3), 0.125),
                point=step["origin"], point_direction=step["direction"], normal=step["normal"], material=step["material"],
                point_time=step["time"], point_state=step["rng_state"])


def advance_arguments(a, direct):
    kw = dict(times=a["time"], rng_state=a["rng_state"], throughput=a["throughput"], ray_id=a["ray_id"], alive=a["alive"], radiance=a["radiance"])
    return dict(kw, scatter_pdf=a["scatter_pdf"], strategy=1, sample=True) if direct else kw


# family -> the call of Scene on the arrays of batch(), every output wanted
FAMILIES = {
    "intersect": lambda s, a, stats: s.intersect(a["origin"], a["direction"], times=a["time"], want=tuple(_lib.QUERY_OUTPUTS), stats=stats),
    "radiance": lambda s, a, stats: s.radiance(a["origin"], a["direction"], times=a["time"], rng_state=a["rng_state"], samples=2, max_depth=6,
                                               want=tuple(_lib.RADIANCE_OUTPUTS), stats=stats),
    "radiance direct": lambda s, a, stats: s.radiance(a["origin"], a["direction"], times=a["time"], rng_state=a["rng_state"], samples=2, max_depth=6,
                                                      want=tuple(_lib.RADIANCE_OUTPUTS), stats=stats, direct="mis", strategy=1),
    "path step": lambda s, a, stats: s.path_step(a["origin"], a["direction"], times=a["time"], rng_state=a["rng_state"], want=tuple(_lib.STEP_OUTPUTS),
                                                 stats=stats),
    "sample lights": lambda s, a, stats: s.sample_lights(a["point"], a["normal"], a["material"], a["point_time"], a["point_state"], strategy=1,
                                                         want=tuple(_lib.LIGHT_SAMPLE_OUTPUTS), stats=stats),
    "light pdf": lambda s, a, stats: s.light_pdf(a["point"], a["point_direction"], times=a["point_time"], strategy=1, want=tuple(_lib.LIGHT_PDF_OUTPUTS),
                                                 stats=stats),
    "path advance": lambda s, a, stats: s.path_advance(a["origin"], a["direction"], want=PLAIN, stats=stats, **advance_arguments(a, False)),
    "path advance direct": lambda s, a, stats: s.path_advance_direct(a["origin"], a["direction"], want=tuple(_lib.ADVANCE_DIRECT_OUTPUTS), stats=stats,
                                                                     **advance_arguments(a, True)),
}


def counted(st):
    """The statistics but the time."""
    return {name: getattr(st, name) for name, _ in st._fields_ if name != "seconds"}


# ---- 1. host call against device call ----
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "with statistics"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_host_call_and_the_device_call_give_the_same_bits(family, stats):
    scene = scene_of(NAME)
    on_host = batch()
    on_device = {k: to_device(v) for k, v in batch().items()}
    host = FAMILIES[family](scene, on_host, stats)
    device = FAMILIES[family](scene, on_device, stats)
    if stats:
        (host, host_st), (device, device_st) = host, device
        assert counted(host_st) == counted(device_st)
        assert host_st.seconds > 0 and device_st.seconds > 0 and host_st.kernel_vgprs > 0
    assert len(host) >= 2 and set(host) == set(device)
    for name, a in host.items():
        got = device[name]
        assert isinstance(got, torch.Tensor) and got.is_cuda, name
        got = to_host(got, a)
        assert a.shape == got.shape and a.shape[0] > 0, (name, a.shape, got.shape)
        assert np.array_equal(bits(a), bits(got)), name
    for name, a in on_host.items():   # the inputs are only read; the advances fold into `radiance` in place
        assert np.array_equal(bits(a), bits(to_host(on_device[name], a))), name
    fresh = batch()
    folded = not np.array_equal(on_host["radiance"], fresh.pop("radiance"))
    assert folded == family.startswith("path advance")
    assert all(np.array_equal(bits(a), bits(on_host[name])) for name, a in fresh.items())


# ---- 2. the occlusion mode of the host call ----
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "with statistics"])
def test_an_occlusion_query_on_host_arrays_writes_occluded_alone(stats):
    scene = scene_of(NAME)
    a = batch()
    outs = {name: np.full((ROWS,) + tail, GUARDS[dtype], dtype=dtype) for name, (dtype, tail) in _lib.QUERY_OUTPUTS.items()}
    p = _lib.QueryParams(ROWS, 0.001, float("inf"), 0.0, SEED, 0, 1, 0, 0, None)
    rays = _lib.QueryRays(a["origin"].ctypes.data, a["direction"].ctypes.data, a["time"].ctypes.data, None, None)
    hits = _lib.QueryHits(**{name: o.ctypes.data for name, o in outs.items()})
    st = _lib.QueryStats()
    status = api.lib().rt_scene_intersect(scene._p, C.byref(p), C.byref(rays), C.byref(hits), C.byref(st) if stats else None)
    assert status == 0, api.lib().rt_last_error().decode()
    want = scene.intersect(a["origin"], a["direction"], times=a["time"], want=("occluded",))["occluded"]
    assert np.array_equal(outs["occluded"], want) and 0 < want.sum() < ROWS
    for name, (dtype, _) in _lib.QUERY_OUTPUTS.items():
        if name != "occluded":
            assert (outs[name] == np.array(GUARDS[dtype]).astype(dtype)).all(), name
    if stats:
        assert st.rays == ROWS and st.hits == want.sum()


# ---- 3. the advances' host call with an input count word ----
def host_advance(direct, scene, a, capacity, said, outs):
    """rt_scene_path_advance or rt_scene_path_advance_direct on the numpy arrays of `a` with rays->count pointing at a host word
    holding `said` (None: no word); `a["radiance"]` is folded into in place.  Returns *out->count."""
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    word = None if said is None else np.array([said], dtype=np.uint32)
    live = np.array([0x5A5A5A5A], dtype=np.uint32)
    params = (capacity, len(a["radiance"]), 0.0, SEED, 0, 0, 0, None, None, 0)
    ray_arrays = tuple(ptr(a[k]) for k in RAY + ("alive",)) + (ptr(word),)
    out_arrays = (ptr(a["radiance"]),) + tuple(ptr(outs[k]) for k in PLAIN) + (ptr(live),)
    if direct:
        p = _lib.PathAdvanceDirectParams(*params, (C.c_int32 * 4)(), 1, 1)
        rays, out = _lib.PathAdvanceDirectRays(*ray_arrays, ptr(a["scatter_pdf"])), _lib.PathAdvanceDirectOut(*out_arrays, ptr(outs["scatter_pdf"]))
        call = api.lib().rt_scene_path_advance_direct
    else:
        p, rays, out = _lib.PathAdvanceParams(*params), _lib.PathAdvanceRays(*ray_arrays), _lib.PathAdvanceOut(*out_arrays)
        call = api.lib().rt_scene_path_advance
    status = call(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    assert status == 0, api.lib().rt_last_error().decode()
    assert word is None or int(word[0]) == said, "the input word is only read"
    return int(live[0])


def guarded(rows, direct):
    table = _lib.ADVANCE_DIRECT_OUTPUTS if direct else _lib.ADVANCE_OUTPUTS
    return {name: np.full((rows,) + tail, GUARDS[dtype], dtype=dtype) for name, (dtype, tail) in table.items()}


@pytest.mark.parametrize("direct", [False, True], ids=["plain", "direct"])
def test_the_host_advance_reads_the_count_word(direct):
    scene = scene_of(NAME)
    capacity = 3 * ROWS
    for said, n in ((130, 130), (capacity + 50, capacity)):   # fewer rows than the capacity; more: clamped
        full, outs = batch(capacity), guarded(capacity, direct)
        alone, alone_outs = {k: np.array(v[:n]) for k, v in full.items()}, guarded(n, direct)
        alone["radiance"] = np.array(full["radiance"])
        want = host_advance(direct, scene, alone, n, None, alone_outs)   # the call on the first n rays alone
        assert 0 < want < n
        assert host_advance(direct, scene, full, capacity, said, outs) == want
        for name in outs:
            assert np.array_equal(bits(outs[name][:want]), bits(alone_outs[name][:want])), (said, name)
        assert np.array_equal(bits(full["radiance"]), bits(alone["radiance"])), "rows at and beyond the word are not stepped"
        assert not np.array_equal(full["radiance"], np.full((capacity, 3), 0.125))
    full, outs = batch(capacity), guarded(capacity, direct)
    assert host_advance(direct, scene, full, capacity, 0, outs) == 0, "a word of 0: no survivors"
    assert np.array_equal(bits(full["radiance"]), bits(batch(capacity)["radiance"]))
    for name, (dtype, _) in (_lib.ADVANCE_DIRECT_OUTPUTS if direct else _lib.ADVANCE_OUTPUTS).items():
        assert (outs[name] == np.array(GUARDS[dtype]).astype(dtype)).all(), name
