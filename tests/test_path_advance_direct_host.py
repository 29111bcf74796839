"""Path advances with light samples (include/rtow.h rt_scene_path_advance_direct): what can be checked without a device -- every
parameter error comes back before the device is touched, in the header's order; an empty batch is no launch; the ctypes structures
have the library's sizes and begin with the plain advance's fields; the workspace is at least the plain call's; and the Python
layer refuses arrays it would have to convert, scatter_pdf included."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
OUTPUTS = ("origin", "direction", "time", "rng_state", "throughput", "ray_id", "t", "normal", "front_face", "material", "scatter_pdf")
INPUTS = ("origin", "direction", "time", "rng_state", "throughput", "ray_id", "scatter_pdf")   # those an output could alias
GUARD = 0xAB   # every byte of every output array before a call


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5))), s.Sphere((0, 3, -3), 0.5, s.DiffuseLight((4, 4, 4)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, sources=1, variant=0, strategy=1, sample=1, origin=True, direction=True, outputs=OUTPUTS, radiance=True,
          out_count=True, alias=None, workspace="enough"):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, the output arrays, message).  A device ordinal
    no machine has: a call that got as far as the device would say so, and the message of a parameter error never mentions the
    device.  `workspace` is a host buffer: no call here gets far enough to touch it."""
    n = max(count, 1) if count <= 4 else 1
    shapes = dict(_lib.ADVANCE_DIRECT_OUTPUTS, radiance=("float64", (3,)), count=("uint32", ()))
    arrays = {name: np.full(n * int(np.prod(tail, dtype=np.int64)) * np.dtype(dtype).itemsize, GUARD, dtype=np.uint8)   # as bytes
              for name, (dtype, tail) in shapes.items()}
    ins = {"origin": np.zeros((n, 3)), "direction": np.tile([0.0, 0.0, -1.0], (n, 1)), "time": np.zeros(n),
           "rng_state": np.zeros((n, 6), dtype=np.uint32), "throughput": np.ones((n, 3)), "ray_id": np.zeros(n, dtype=np.int32),
           "scatter_pdf": np.zeros(n)}
    need = int(api.lib().rt_path_advance_direct_workspace_bytes(min(max(count, 0), 1 << 30)))
    buffer = np.zeros(8192, dtype=np.uint8)
    ws, ws_bytes = {"enough": (buffer.ctypes.data, need), "null": (None, need), "short": (buffer.ctypes.data, need - 1)}[workspace]
    p = _lib.PathAdvanceDirectParams(count, sources, 0.0, 1984, 0, variant, 12345, None, ws, ws_bytes, (C.c_int32 * 4)(), strategy, sample)
    given = {name: ins[name].ctypes.data for name in INPUTS}
    if not origin:
        given["origin"] = None
    if not direction:
        given["direction"] = None
    rays = _lib.PathAdvanceDirectRays(*(given[name] for name in INPUTS[:-1]), None, None, given["scatter_pdf"])
    out = {name: arrays[name].ctypes.data for name in outputs}
    if alias:
        out[alias] = given[alias]
    full = _lib.PathAdvanceDirectOut(arrays["radiance"].ctypes.data if radiance else None, *(out.get(name) for name in _lib.ADVANCE_OUTPUTS),
                                     arrays["count"].ctypes.data if out_count else None, out.get("scatter_pdf"))
    fn = api.lib().rt_scene_path_advance_direct if host else api.lib().rt_scene_path_advance_direct_device
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
    "strategy 2": dict(strategy=2),
    "strategy -1": dict(strategy=-1),
    "sample 2": dict(sample=2),
    "sample -1": dict(sample=-1),
    "null origin": dict(origin=False),
    "null direction": dict(direction=False),
    "null out origin": dict(outputs=tuple(n for n in OUTPUTS if n != "origin")),
    "null out direction": dict(outputs=tuple(n for n in OUTPUTS if n != "direction")),
    "null out count": dict(out_count=False),
    "radiance of no rows": dict(sources=0),
}
ERRORS.update({f"aliased {name}": dict(alias=name) for name in INPUTS})
DEVICE_ERRORS = {"null workspace": dict(workspace="null"), "short workspace": dict(workspace="short")}


def _own(host):
    return "rt_scene_path_advance_direct" + ("" if host else "_device")


def _is_parameter_error(status, arrays, message, host):
    assert status == RT_ERR_INVALID, message
    assert "device" not in message.replace(_own(host), "") and "HIP" not in message, message
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
    assert "rt_path_advance_direct_workspace_bytes" in message
    status, _, message = _call(_scene(), True, **DEVICE_ERRORS[name])   # the host call ignores the workspace
    assert status != RT_OK and ("device" in message or "HIP" in message), message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_valid_parameters_get_as_far_as_the_device(host):
    """The other side of the table: the limits themselves are accepted (the call then fails on device ordinal 12345), and so are
    the required outputs alone, a call without a radiance array, both strategies and both values of the sample switch."""
    cases = [dict(), dict(variant=1), dict(count=1 << 30), dict(sources=1 << 30), dict(outputs=("origin", "direction")), dict(radiance=False),
             dict(radiance=False, sources=0), dict(strategy=0), dict(sample=0), dict(strategy=0, sample=0)]
    for kw in cases:   # (the workspace of 2^30 rows is only named: no call here gets as far as touching it)
        status, _, message = _call(_scene(), host, **kw)
        assert status != RT_OK and ("device" in message.replace(_own(host), "") or "HIP" in message), (kw, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_advance_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    for kw in (dict(count=-1), dict(strategy=5), dict(sample=5), dict(alias="scatter_pdf"), dict(workspace="null")):   # the state first
        status, _, message = _call(_scene(commit=False), host, **kw)
        assert status == RT_ERR_STATE, message


def test_the_refusals_come_in_the_headers_order():
    """Two errors at once: the earlier of the header's list is the one reported.  The strategy and the sample switch come directly
    behind the variant; the new aliased pair stands with the aliased pairs."""
    order = [("count must be", dict(count=-1)), ("sources must be", dict(sources=-1)), ("variant", dict(variant=2)),
             ("strategy must be", dict(strategy=2)), ("sample must be", dict(sample=2)),
             ("null origin or direction", dict(origin=False)), ("are required", dict(out_count=False)),
             ("radiance array of no rows", dict(sources=0)), ("same meaning", dict(alias="scatter_pdf")), ("workspace", dict(workspace="null"))]
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
    for kw in (dict(variant=3), dict(sources=-1), dict(strategy=2), dict(sample=2), dict(out_count=False), dict(alias="scatter_pdf"),
               dict(sources=0)):   # ... but the parameters are still checked
        status, _, _ = _call(_scene(), host, count=0, **kw)
        assert status == RT_ERR_INVALID, kw


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_path_advance_direct_abi_sizes(sizes)
    structs = (_lib.PathAdvanceDirectParams, _lib.PathAdvanceDirectRays, _lib.PathAdvanceDirectOut, _lib.PathAdvanceDirectStats)
    ours = [C.sizeof(x) for x in structs]
    assert list(sizes) == ours
    assert ours == [96, 72, 104, 56]   # include/rtow.h on LP64: the plain advance's 88 / 64 / 96 and 2 x 4 / a pointer / a pointer; 5 x 8 + 4 x 4
    plain = (_lib.PathAdvanceParams, _lib.PathAdvanceRays, _lib.PathAdvanceOut)
    added = (["strategy", "sample"], ["scatter_pdf"], ["scatter_pdf"])
    for ours_, theirs, more in zip(structs, plain, added):   # the plain advance's fields, at the plain advance's offsets, then the new ones
        assert [name for name, _ in ours_._fields_] == [name for name, _ in theirs._fields_] + more
        for name, _ in theirs._fields_:
            assert getattr(ours_, name).offset == getattr(theirs, name).offset, name
    assert list(_lib.ADVANCE_DIRECT_OUTPUTS) == list(OUTPUTS) and list(_lib.ADVANCE_DIRECT_OUTPUTS)[:-1] == list(_lib.ADVANCE_OUTPUTS)
    assert _lib.ADVANCE_DIRECT_OUTPUTS["scatter_pdf"] == ("float64", ())
    assert [name for name, _ in _lib.PathAdvanceDirectStats._fields_] == ["rays", "scattered", "shadow_rays", "shadow_reached", "seconds",
                                                                          "kernel_vgprs", "scratch_bytes", "shadow_vgprs", "shadow_scratch_bytes"]


def test_the_workspace_is_nothing_for_nothing_grows_with_the_count_and_holds_the_plain_calls():
    size, plain = api.lib().rt_path_advance_direct_workspace_bytes, api.lib().rt_path_advance_workspace_bytes
    assert size(0) == 0
    counts = [1, 63, 64, 65, 256, 257, 1 << 20, 1 << 30]
    sizes = [size(n) for n in counts]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(size(n) >= plain(n) for n in counts)
    assert sizes[-1] > 1 << 32, "a size that needs its 64 bits"


def test_python_reports_the_librarys_errors():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    with pytest.raises(rt.RtowError) as info:
        s.path_advance_direct(o, d, device=12345, variant=2)
    assert "status 1" in str(info.value) and "device" not in str(info.value), str(info.value)
    with pytest.raises(rt.RtowError) as info:
        _scene(commit=False).path_advance_direct(o, d, device=12345)
    assert "status 5" in str(info.value)
    with pytest.raises(rt.RtowError) as info:
        s.path_advance_direct(o, d, device=12345, strategy=2)
    assert "strategy" in str(info.value)


def test_python_refuses_arrays_it_would_have_to_convert():
    torch = pytest.importorskip("torch")
    s = _scene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1))
    state = np.zeros((4, 6), dtype=np.uint32)
    cases = {
        "float32 origins": (o.astype(np.float32), d, {}),
        "strided directions": (o, np.asfortranarray(d), {}),
        "counts differ": (o, d[:3].copy(), {}),
        "a scalar for times": (o, d, dict(times=0.5)),
        "64-bit state words": (o, d, dict(rng_state=state.astype(np.uint64))),
        "float32 throughput": (o, d, dict(throughput=np.ones((4, 3), dtype=np.float32))),
        "64-bit ids": (o, d, dict(ray_id=np.arange(4))),
        "bool alive": (o, d, dict(alive=np.ones(4, dtype=bool))),
        "float32 radiance": (o, d, dict(radiance=np.zeros((4, 3), dtype=np.float32))),
        "float32 scatter_pdf": (o, d, dict(scatter_pdf=np.zeros(4, dtype=np.float32))),
        "scatter_pdf of three channels": (o, d, dict(scatter_pdf=np.zeros((4, 3)))),
        "scatter_pdf of another length": (o, d, dict(scatter_pdf=np.zeros(5))),
        "strided scatter_pdf": (o, d, dict(scatter_pdf=np.zeros(8)[::2])),
        "a scalar for scatter_pdf": (o, d, dict(scatter_pdf=0.0)),
        "a tensor for scatter_pdf": (o, d, dict(scatter_pdf=torch.zeros(4, dtype=torch.float64))),
        "unknown output": (o, d, dict(want=("origin", "status"))),
    }
    for name, (origins, directions, kw) in cases.items():
        with pytest.raises(rt.RtowError):
            s.path_advance_direct(origins, directions, device=12345, **kw)
            pytest.fail(name + " was accepted")
    with pytest.raises(rt.RtowError):   # torch tensors must live on the GPU
        s.path_advance_direct(torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(rt.RtowError):
        rt.PathBatch(s, o, d, direct="mis")   # PathBatch takes CUDA tensors only
    with pytest.raises(rt.RtowError) as info:   # what is accepted gets as far as the device
        s.path_advance_direct(o, d, times=np.zeros(4), rng_state=state, throughput=np.ones((4, 3)), ray_id=np.arange(4, dtype=np.int32),
                              alive=np.ones(4, dtype=np.uint8), radiance=np.zeros((4, 3)), scatter_pdf=np.zeros(4), want=OUTPUTS, device=12345)
    assert "device" in str(info.value) or "HIP" in str(info.value)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    radiance = np.full((2, 3), 7.0)
    out = s.path_advance_direct(np.zeros((0, 3)), np.zeros((0, 3)), radiance=radiance, want=OUTPUTS)
    assert list(out) == list(OUTPUTS)
    for name, (dtype, tail) in _lib.ADVANCE_DIRECT_OUTPUTS.items():
        assert out[name].shape == (0,) + tail and out[name].dtype == np.dtype(dtype), name
    assert (radiance == 7.0).all()
    out, st = s.path_advance_direct(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)
    assert list(out) == ["origin", "direction", "time", "rng_state", "throughput", "ray_id", "scatter_pdf"]
    assert st.rays == 0 and st.scattered == 0 and st.shadow_rays == 0 and st.shadow_reached == 0 and st.seconds == 0.0
