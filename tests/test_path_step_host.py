"""Path steps (include/rtow.h rt_scene_path_step): what can be checked without a device -- every parameter error comes back before
the device is touched, an empty batch is no launch, the ctypes structures have the library's sizes, and the Python layer refuses
arrays it would have to convert."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
OUTPUTS = ("status", "emitted", "attenuation", "origin", "direction", "time", "t", "normal", "front_face", "material", "rng_state")
GUARD = 0xAB   # every byte of every output array before a call


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, variant=0, origin=True, direction=True, outputs=OUTPUTS):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, the output arrays, message).  A device ordinal
    no machine has: a call that got as far as the device would say so, and the message of a parameter error never mentions the
    device."""
    n = max(count, 1) if count <= 4 else 1
    o = np.zeros((n, 3))
    d = np.tile([0.0, 0.0, -1.0], (n, 1))
    arrays = {name: np.full(n * int(np.prod(tail, dtype=np.int64)) * np.dtype(dtype).itemsize, GUARD, dtype=np.uint8)   # as bytes
              for name, (dtype, tail) in _lib.STEP_OUTPUTS.items()}
    p = _lib.PathStepParams(count, 0.0, 1984, 0, variant, 12345, None)
    rays = _lib.PathStepRays(o.ctypes.data if origin else None, d.ctypes.data if direction else None, None, None)
    out = _lib.PathStepOut(**{name: arrays[name].ctypes.data for name in outputs})
    fn = api.lib().rt_scene_path_step if host else api.lib().rt_scene_path_step_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _untouched(arrays):
    return all((a == GUARD).all() for a in arrays.values())


# the refusal table of include/rtow.h
ERRORS = {
    "negative count": dict(count=-1),
    "count above 2^30": dict(count=(1 << 30) + 1),
    "variant 2": dict(variant=2),
    "variant -1": dict(variant=-1),
    "null origin": dict(origin=False),
    "null direction": dict(direction=False),
    "all outputs null": dict(outputs=()),
}


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_parameter_errors_come_back_before_the_device_is_touched(name, host):
    status, arrays, message = _call(_scene(), host, **ERRORS[name])
    assert status == RT_ERR_INVALID, message
    assert "device" not in message.replace("rt_scene_path_step_device", "") and "HIP" not in message, message
    assert _untouched(arrays), "nothing was written"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_valid_parameters_get_as_far_as_the_device(host):
    """The other side of the table: the limits themselves are accepted (the call then fails on device ordinal 12345), and so is
    every output alone."""
    for kw in [dict(), dict(variant=1), dict(count=1 << 30)] + [dict(outputs=(name,)) for name in OUTPUTS]:
        status, _, message = _call(_scene(), host, **kw)
        assert status != RT_OK and ("device" in message.replace("rt_scene_path_step_device", "") or "HIP" in message), (kw, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_a_step_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    status, _, message = _call(_scene(commit=False), host, count=-1)   # the order of include/rtow.h: the state first
    assert status == RT_ERR_STATE, message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_empty_batch_is_ok_without_a_launch(host):
    status, arrays, message = _call(_scene(), host, count=0)
    assert status == RT_OK, message
    assert _untouched(arrays)
    status, _, message = _call(_scene(), host, count=0, origin=False, direction=False)   # no rays: no arrays needed
    assert status == RT_OK, message
    for kw in (dict(variant=3), dict(outputs=())):   # ... but the parameters are still checked
        status, _, _ = _call(_scene(), host, count=0, **kw)
        assert status == RT_ERR_INVALID, kw


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_path_step_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.PathStepParams, _lib.PathStepRays, _lib.PathStepOut, _lib.PathStepStats)]
    assert list(sizes) == ours
    assert ours == [64, 32, 88, 32]   # include/rtow.h on LP64: 4 x 8 + 2 x 4 + 8 + 16; 4 and 11 pointers; 3 x 8 + 2 x 4
    assert [name for name, _ in _lib.PathStepOut._fields_] == list(OUTPUTS) == list(_lib.STEP_OUTPUTS)
    assert [name for name, _ in _lib.PathStepRays._fields_] == ["origin", "direction", "time", "rng_state"]
    assert [name for name, _ in _lib.PathStepParams._fields_] == ["count", "time", "seed", "first_sequence", "variant", "device", "stream", "reserved"]
    assert [name for name, _ in _lib.PathStepStats._fields_] == ["rays", "scattered", "seconds", "kernel_vgprs", "scratch_bytes"]


def test_python_reports_the_librarys_errors():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    with pytest.raises(rt.RtowError) as info:
        s.path_step(o, d, device=12345, variant=2)
    assert "status 1" in str(info.value) and "device" not in str(info.value), str(info.value)
    with pytest.raises(rt.RtowError) as info:
        _scene(commit=False).path_step(o, d, device=12345)
    assert "status 5" in str(info.value)


def test_python_refuses_arrays_it_would_have_to_convert():
    s = _scene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1))
    state = np.zeros((4, 6), dtype=np.uint32)
    cases = {
        "float32 origins": (o.astype(np.float32), d, {}),
        "float32 directions": (o, d.astype(np.float32), {}),
        "strided origins": (np.zeros((4, 6))[:, ::2], d, {}),
        "strided directions": (o, np.asfortranarray(d), {}),
        "a list": (o.tolist(), d, {}),
        "wrong trailing shape": (np.zeros((4, 2)), d, {}),
        "counts differ": (o, d[:3].copy(), {}),
        "float32 times": (o, d, dict(times=np.zeros(4, dtype=np.float32))),
        "times of another length": (o, d, dict(times=np.zeros(5))),
        "a scalar for times": (o, d, dict(times=0.5)),
        "64-bit state words": (o, d, dict(rng_state=state.astype(np.uint64))),
        "float state words": (o, d, dict(rng_state=state.astype(np.float64))),
        "five state words": (o, d, dict(rng_state=np.zeros((4, 5), dtype=np.uint32))),
        "state in planes": (o, d, dict(rng_state=np.zeros((6, 4), dtype=np.uint32))),
        "strided state": (o, d, dict(rng_state=np.zeros((4, 12), dtype=np.uint32)[:, ::2])),
        "state of another length": (o, d, dict(rng_state=np.zeros((3, 6), dtype=np.uint32))),
        "unknown output": (o, d, dict(want=("status", "radiance"))),
        "no output": (o, d, dict(want=())),
    }
    for name, (origins, directions, kw) in cases.items():
        with pytest.raises(rt.RtowError):
            s.path_step(origins, directions, device=12345, **kw)
            pytest.fail(name + " was accepted")
    with pytest.raises(rt.RtowError) as info:   # what is accepted gets as far as the device
        s.path_step(o, d, times=np.zeros(4), rng_state=state, want=OUTPUTS, device=12345)
    assert "device" in str(info.value) or "HIP" in str(info.value)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    out = s.path_step(np.zeros((0, 3)), np.zeros((0, 3)), want=OUTPUTS)
    assert list(out) == list(OUTPUTS)
    for name, (dtype, tail) in _lib.STEP_OUTPUTS.items():
        assert out[name].shape == (0,) + tail and out[name].dtype == np.dtype(dtype), name
    out, st = s.path_step(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)
    assert list(out) == ["status", "emitted", "attenuation", "origin", "direction", "time", "rng_state"]
    assert st.rays == 0 and st.scattered == 0 and st.seconds == 0.0
