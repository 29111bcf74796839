"""Path advances (include/rtow.h rt_scene_path_advance): what can be checked without a device -- every parameter error comes back
before the device is touched, in the header's order; an empty batch is no launch; the ctypes structures have the library's sizes;
the workspace size grows with the count; and the Python layer refuses arrays it would have to convert."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
OUTPUTS = ("origin", "direction", "time", "rng_state", "throughput", "ray_id", "t", "normal", "front_face", "material")
INPUTS = ("origin", "direction", "time", "rng_state", "throughput", "ray_id")   # those an output could alias
GUARD = 0xAB   # every byte of every output array before a call


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, sources=1, variant=0, origin=True, direction=True, outputs=OUTPUTS, radiance=True, out_count=True, alias=None,
          workspace="enough"):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, the output arrays, message).  A device ordinal
    no machine has: a call that got as far as the device would say so, and the message of a parameter error never mentions the
    device.  `workspace` is a host buffer: no call here gets far enough to touch it."""
    n = max(count, 1) if count <= 4 else 1
    shapes = dict(_lib.ADVANCE_OUTPUTS, radiance=("float64", (3,)), count=("uint32", ()))
    arrays = {name: np.full(n * int(np.prod(tail, dtype=np.int64)) * np.dtype(dtype).itemsize, GUARD, dtype=np.uint8)   # as bytes
              for name, (dtype, tail) in shapes.items()}
    ins = {"origin": np.zeros((n, 3)), "direction": np.tile([0.0, 0.0, -1.0], (n, 1)), "time": np.zeros(n),
           "rng_state": np.zeros((n, 6), dtype=np.uint32), "throughput": np.ones((n, 3)), "ray_id": np.zeros(n, dtype=np.int32)}
    need = int(api.lib().rt_path_advance_workspace_bytes(min(max(count, 0), 1 << 30)))
    buffer = np.zeros(4096, dtype=np.uint8)
    ws, ws_bytes = {"enough": (buffer.ctypes.data, need), "null": (None, need), "short": (buffer.ctypes.data, need - 1)}[workspace]
    p = _lib.PathAdvanceParams(count, sources, 0.0, 1984, 0, variant, 12345, None, ws, ws_bytes)
    given = {name: ins[name].ctypes.data for name in INPUTS}
    if not origin:
        given["origin"] = None
    if not direction:
        given["direction"] = None
    rays = _lib.PathAdvanceRays(*(given[name] for name in INPUTS), None, None)
    out = {name: arrays[name].ctypes.data for name in outputs}
    if alias:
        out[alias] = given[alias]
    full = _lib.PathAdvanceOut(arrays["radiance"].ctypes.data if radiance else None, *(out.get(name) for name in _lib.ADVANCE_OUTPUTS),
                               arrays["count"].ctypes.data if out_count else None)
    fn = api.lib().rt_scene_path_advance if host else api.lib().rt_scene_path_advance_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(full), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _untouched(arrays):
    return all((a == GUARD).all() for a in arrays.values())


# the refusal table of include/rtow.h
ERRORS = {
    "negative count": dict(count=-1),
    "count above 2^30": dict(count=(1 << 30) + 1),
    "negative sources": dict(sources=-1),
    "sources above 2^30": dict(sources=(1 << 30) + 1),
    "variant 2": dict(variant=2),
    "variant -1": dict(variant=-1),
    "null origin": dict(origin=False),
    "null direction": dict(direction=False),
    "null out origin": dict(outputs=tuple(n for n in OUTPUTS if n != "origin")),
    "null out direction": dict(outputs=tuple(n for n in OUTPUTS if n != "direction")),
    "null out count": dict(out_count=False),
    "radiance of no rows": dict(sources=0),
}
ERRORS.update({f"aliased {name}": dict(alias=name) for name in INPUTS})
DEVICE_ERRORS = {"null workspace": dict(workspace="null"), "short workspace": dict(workspace="short")}


def _is_parameter_error(status, arrays, message, host):
    assert status == RT_ERR_INVALID, message
    own = "rt_scene_path_advance" + ("" if host else "_device")
    assert "device" not in message.replace(own, "") and "HIP" not in message, message
    assert _untouched(arrays), "nothing was written"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_parameter_errors_come_back_before_the_device_is_touched(name, host):
    status, arrays, message = _call(_scene(), host, **ERRORS[name])
    _is_parameter_error(status, arrays, message, host)


@pytest.mark.parametrize("name", sorted(DEVICE_ERRORS))
def test_the_device_call_refuses_a_workspace_it_cannot_use(name):
    status, arrays, message = _call(_scene(), False, **DEVICE_ERRORS[name])
    _is_parameter_error(status, arrays, message, False)
    status, _, message = _call(_scene(), True, **DEVICE_ERRORS[name])   # the host call ignores the workspace
    assert status != RT_OK and ("device" in message or "HIP" in message), message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_valid_parameters_get_as_far_as_the_device(host):
    """The other side of the table: the limits themselves are accepted (the call then fails on device ordinal 12345), and so are
    the required outputs alone and a call without a radiance array."""
    cases = [dict(), dict(variant=1), dict(count=1 << 30), dict(sources=1 << 30), dict(outputs=("origin", "direction")), dict(radiance=False),
             dict(radiance=False, sources=0)]
    for kw in cases:   # (the workspace of 2^30 rows is only named: no call here gets as far as touching it)
        status, _, message = _call(_scene(), host, **kw)
        own = "rt_scene_path_advance" + ("" if host else "_device")
        assert status != RT_OK and ("device" in message.replace(own, "") or "HIP" in message), (kw, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_advance_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    for kw in (dict(count=-1), dict(alias="origin"), dict(workspace="null")):   # the order of include/rtow.h: the state first
        status, _, message = _call(_scene(commit=False), host, **kw)
        assert status == RT_ERR_STATE, message


def test_the_refusals_come_in_the_headers_order():
    """Two errors at once: the earlier of the header's list is the one reported."""
    order = [("count must be", dict(count=-1)), ("sources must be", dict(sources=-1)), ("variant", dict(variant=2)),
             ("null origin or direction", dict(origin=False)), ("are required", dict(out_count=False)),
             ("radiance array of no rows", dict(sources=0)), ("same meaning", dict(alias="time")), ("workspace", dict(workspace="null"))]
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kw = dict(order[b][1], **order[a][1])
            if "sources" in order[a][1] and "sources" in order[b][1]:
                continue
            status, arrays, message = _call(_scene(), False, **kw)
            assert status == RT_ERR_INVALID and order[a][0] in message, (kw, message)
            assert _untouched(arrays)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_empty_batch_is_ok_without_a_launch(host):
    status, arrays, message = _call(_scene(), host, count=0)
    assert status == RT_OK, message
    assert _untouched(arrays), "not even the count word is written"
    status, _, message = _call(_scene(), host, count=0, origin=False, direction=False, workspace="null")   # no rays: no arrays, no workspace
    assert status == RT_OK, message
    for kw in (dict(variant=3), dict(sources=-1), dict(out_count=False), dict(alias="rng_state"), dict(sources=0)):   # ... but the parameters are still checked
        status, _, _ = _call(_scene(), host, count=0, **kw)
        assert status == RT_ERR_INVALID, kw


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_path_advance_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.PathAdvanceParams, _lib.PathAdvanceRays, _lib.PathAdvanceOut, _lib.PathAdvanceStats)]
    assert list(sizes) == ours
    assert ours == [88, 64, 96, 32]   # include/rtow.h on LP64: 5 x 8 + 2 x 4 + 3 x 8 + 16; 8 and 12 pointers; 3 x 8 + 2 x 4
    assert [name for name, _ in _lib.PathAdvanceOut._fields_] == ["radiance"] + list(OUTPUTS) + ["count"]
    assert list(_lib.ADVANCE_OUTPUTS) == list(OUTPUTS)
    assert [name for name, _ in _lib.PathAdvanceRays._fields_] == ["origin", "direction", "time", "rng_state", "throughput", "ray_id", "alive", "count"]
    assert [name for name, _ in _lib.PathAdvanceParams._fields_] == ["count", "sources", "time", "seed", "first_sequence", "variant", "device", "stream",
                                                                     "workspace", "workspace_bytes", "reserved"]
    assert [name for name, _ in _lib.PathAdvanceStats._fields_] == ["rays", "scattered", "seconds", "kernel_vgprs", "scratch_bytes"]


def test_the_workspace_is_nothing_for_nothing_and_grows_with_the_count():
    size = api.lib().rt_path_advance_workspace_bytes
    assert size(0) == 0
    counts = [1, 63, 64, 65, 256, 257, 1 << 20, 1 << 30]
    sizes = [size(n) for n in counts]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[-1] > 1 << 32, "a size that needs its 64 bits"


def test_python_reports_the_librarys_errors():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    with pytest.raises(rt.RtowError) as info:
        s.path_advance(o, d, device=12345, variant=2)
    assert "status 1" in str(info.value) and "device" not in str(info.value), str(info.value)
    with pytest.raises(rt.RtowError) as info:
        _scene(commit=False).path_advance(o, d, device=12345)
    assert "status 5" in str(info.value)


def test_python_refuses_arrays_it_would_have_to_convert():
    torch = pytest.importorskip("torch")
    s = _scene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1))
    state = np.zeros((4, 6), dtype=np.uint32)
    cases = {
        "float32 origins": (o.astype(np.float32), d, {}),
        "strided directions": (o, np.asfortranarray(d), {}),
        "a list": (o.tolist(), d, {}),
        "wrong trailing shape": (np.zeros((4, 2)), d, {}),
        "counts differ": (o, d[:3].copy(), {}),
        "float32 times": (o, d, dict(times=np.zeros(4, dtype=np.float32))),
        "a scalar for times": (o, d, dict(times=0.5)),
        "64-bit state words": (o, d, dict(rng_state=state.astype(np.uint64))),
        "strided state": (o, d, dict(rng_state=np.zeros((4, 12), dtype=np.uint32)[:, ::2])),
        "float32 throughput": (o, d, dict(throughput=np.ones((4, 3), dtype=np.float32))),
        "throughput of one channel": (o, d, dict(throughput=np.ones(4))),
        "throughput of another length": (o, d, dict(throughput=np.ones((5, 3)))),
        "64-bit ids": (o, d, dict(ray_id=np.arange(4))),
        "unsigned ids": (o, d, dict(ray_id=np.arange(4, dtype=np.uint32))),
        "bool alive": (o, d, dict(alive=np.ones(4, dtype=bool))),
        "alive of another length": (o, d, dict(alive=np.ones(3, dtype=np.uint8))),
        "float32 radiance": (o, d, dict(radiance=np.zeros((4, 3), dtype=np.float32))),
        "radiance in planes": (o, d, dict(radiance=np.zeros((3, 4)))),
        "strided radiance": (o, d, dict(radiance=np.zeros((4, 6))[:, ::2])),
        "a tensor beside numpy arrays": (o, d, dict(radiance=torch.zeros((4, 3), dtype=torch.float64))),
        "a tensor for the ids": (o, d, dict(ray_id=torch.arange(4, dtype=torch.int32))),
        "unknown output": (o, d, dict(want=("origin", "status"))),
    }
    for name, (origins, directions, kw) in cases.items():
        with pytest.raises(rt.RtowError):
            s.path_advance(origins, directions, device=12345, **kw)
            pytest.fail(name + " was accepted")
    with pytest.raises(rt.RtowError):   # torch tensors must live on the GPU
        s.path_advance(torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(rt.RtowError):
        rt.PathBatch(s, o, d)   # PathBatch takes CUDA tensors only
    with pytest.raises(rt.RtowError) as info:   # what is accepted gets as far as the device
        s.path_advance(o, d, times=np.zeros(4), rng_state=state, throughput=np.ones((4, 3)), ray_id=np.arange(4, dtype=np.int32),
                       alive=np.ones(4, dtype=np.uint8), radiance=np.zeros((4, 3)), want=OUTPUTS, device=12345)
    assert "device" in str(info.value) or "HIP" in str(info.value)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    radiance = np.full((2, 3), 7.0)
    out = s.path_advance(np.zeros((0, 3)), np.zeros((0, 3)), radiance=radiance, want=OUTPUTS)
    assert list(out) == list(OUTPUTS)
    for name, (dtype, tail) in _lib.ADVANCE_OUTPUTS.items():
        assert out[name].shape == (0,) + tail and out[name].dtype == np.dtype(dtype), name
    assert (radiance == 7.0).all()
    out, st = s.path_advance(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)
    assert list(out) == ["origin", "direction", "time", "rng_state", "throughput", "ray_id"]
    assert st.rays == 0 and st.scattered == 0 and st.seconds == 0.0
