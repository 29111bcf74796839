"""Radiance queries (include/rtow.h rt_scene_radiance): what can be checked without a device -- every parameter error comes back
before the device is touched, an empty batch is no launch, the ctypes structures have the library's sizes, and the Python layer
refuses arrays it would have to convert."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
OUTPUTS = ("radiance", "path_rays", "rng_state")


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, samples=1, max_depth=50, variant=0, origin=True, direction=True, outputs=OUTPUTS):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, the output arrays, message).  A device ordinal
    no machine has: a call that got as far as the device would say so (RT_ERR_NO_DEVICE or RT_ERR_INVALID 'device ordinal'), and
    the message of a parameter error never mentions the device."""
    n = max(count, 1) if count <= 4 else 1
    o = np.zeros((n, 3))
    d = np.tile([0.0, 0.0, -1.0], (n, 1))
    arrays = {"radiance": np.full((n, 3), -1.0), "path_rays": np.full(n, 0xABCDEF, dtype=np.uint32),
              "rng_state": np.full((n, 6), 0xABCDEF, dtype=np.uint32)}
    p = _lib.RadianceParams(count, samples, max_depth, 0.0, 1984, 0, variant, 12345, None)
    rays = _lib.RadianceRays(o.ctypes.data if origin else None, d.ctypes.data if direction else None, None, None)
    out = _lib.RadianceOut(**{name: arrays[name].ctypes.data for name in outputs})
    fn = api.lib().rt_scene_radiance if host else api.lib().rt_scene_radiance_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _untouched(arrays):
    return (arrays["radiance"] == -1.0).all() and (arrays["path_rays"] == 0xABCDEF).all() and (arrays["rng_state"] == 0xABCDEF).all()


ERRORS = {
    "negative count": dict(count=-1),
    "count above 2^30": dict(count=(1 << 30) + 1),
    "samples 0": dict(samples=0),
    "samples -3": dict(samples=-3),
    "samples above 2^20": dict(samples=(1 << 20) + 1),
    "max_depth -1": dict(max_depth=-1),
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
    assert "device" not in message.replace("rt_scene_radiance_device", "") and "HIP" not in message, message
    assert _untouched(arrays), "nothing was written"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_valid_parameters_get_as_far_as_the_device(host):
    """The other side of the table: the limits themselves are accepted (the call then fails on device ordinal 12345)."""
    for kw in (dict(), dict(samples=1 << 20), dict(max_depth=0), dict(variant=1), dict(count=1 << 30), dict(outputs=("path_rays",))):
        status, _, message = _call(_scene(), host, **kw)
        assert status != RT_OK and ("device" in message.replace("rt_scene_radiance_device", "") or "HIP" in message), (kw, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_a_query_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    status, _, message = _call(_scene(commit=False), host, samples=0)   # the order of include/rtow.h: the state first
    assert status == RT_ERR_STATE, message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_empty_batch_is_ok_without_a_launch(host):
    status, arrays, message = _call(_scene(), host, count=0)
    assert status == RT_OK, message
    assert _untouched(arrays)
    status, _, message = _call(_scene(), host, count=0, origin=False, direction=False)   # no rays: no arrays needed
    assert status == RT_OK, message
    for kw in (dict(samples=0), dict(max_depth=-1), dict(variant=3), dict(outputs=())):   # ... but the parameters are still checked
        status, _, _ = _call(_scene(), host, count=0, **kw)
        assert status == RT_ERR_INVALID, kw


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_radiance_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.RadianceParams, _lib.RadianceRays, _lib.RadianceOut, _lib.RadianceStats)]
    assert list(sizes) == ours
    assert ours == [72, 32, 24, 24]   # include/rtow.h on LP64: 8 + 2 x 4 + 8 + 2 x 8 + 2 x 4 + 8 + 16; 4 and 3 pointers; 8 + 8 + 2 x 4
    assert [name for name, _ in _lib.RadianceOut._fields_] == list(OUTPUTS)
    assert [name for name, _ in _lib.RadianceRays._fields_] == ["origin", "direction", "time", "rng_state"]


def test_python_reports_the_librarys_errors():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    for kw in (dict(samples=0), dict(samples=(1 << 20) + 1), dict(max_depth=-1), dict(variant=2)):
        with pytest.raises(rt.RtowError) as info:
            s.radiance(o, d, device=12345, **kw)
        assert "status 1" in str(info.value) and "device" not in str(info.value), (kw, str(info.value))
    with pytest.raises(rt.RtowError) as info:
        _scene(commit=False).radiance(o, d, device=12345)
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
        "unknown output": (o, d, dict(want=("radiance", "colour"))),
        "no output": (o, d, dict(want=())),
        "fractional samples": (o, d, dict(samples=1.5)),
    }
    for name, (origins, directions, kw) in cases.items():
        with pytest.raises(rt.RtowError):
            s.radiance(origins, directions, device=12345, **kw)
            pytest.fail(name + " was accepted")
    assert np.zeros((4, 6))[:, ::2].shape == (4, 3) and not np.asfortranarray(d).flags.c_contiguous   # (the cases are what they say)
    with pytest.raises(rt.RtowError) as info:   # what is accepted gets as far as the device
        s.radiance(o, d, times=np.zeros(4), rng_state=state, want=OUTPUTS, device=12345)
    assert "device" in str(info.value) or "HIP" in str(info.value)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    out = s.radiance(np.zeros((0, 3)), np.zeros((0, 3)), want=OUTPUTS)
    assert sorted(out) == sorted(OUTPUTS)
    assert out["radiance"].shape == (0, 3) and out["radiance"].dtype == np.float64
    assert out["path_rays"].shape == (0,) and out["path_rays"].dtype == np.uint32
    assert out["rng_state"].shape == (0, 6) and out["rng_state"].dtype == np.uint32
    out, st = s.radiance(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)
    assert list(out) == ["radiance"] and st.rays == 0 and st.seconds == 0.0
