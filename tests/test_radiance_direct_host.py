"""Radiance queries with light samples (include/rtow.h rt_scene_radiance_direct): what can be checked without a device -- every
parameter error comes back before the device is touched, in the header's order (rt_scene_radiance's, then the strategy); an empty
batch is no launch; the ctypes structures have the library's sizes and begin with the plain call's fields; and Scene.radiance
accepts direct=None and direct="mis" and refuses everything else."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
OUTPUTS = ("radiance", "path_rays", "rng_state")
NAMES = ("rt_scene_radiance_direct_device", "rt_scene_radiance_direct")


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5))), s.Sphere((0, 3, -3), 0.5, s.DiffuseLight((4, 4, 4)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, samples=1, max_depth=50, variant=0, strategy=1, origin=True, direction=True, outputs=OUTPUTS):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, the output arrays, message).  A device ordinal
    no machine has: a call that got as far as the device would say so, and the message of a parameter error never mentions the
    device."""
    n = max(count, 1) if count <= 4 else 1
    o = np.zeros((n, 3))
    d = np.tile([0.0, 0.0, -1.0], (n, 1))
    arrays = {"radiance": np.full((n, 3), -1.0), "path_rays": np.full(n, 0xABCDEF, dtype=np.uint32),
              "rng_state": np.full((n, 6), 0xABCDEF, dtype=np.uint32)}
    p = _lib.RadianceDirectParams(count, samples, max_depth, 0.0, 1984, 0, variant, 12345, None, (C.c_int32 * 4)(), strategy)
    rays = _lib.RadianceRays(o.ctypes.data if origin else None, d.ctypes.data if direction else None, None, None)
    out = _lib.RadianceOut(**{name: arrays[name].ctypes.data for name in outputs})
    fn = api.lib().rt_scene_radiance_direct if host else api.lib().rt_scene_radiance_direct_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _names_no_device(message):
    for name in NAMES:
        message = message.replace(name, "")
    return "device" not in message and "HIP" not in message


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
    "strategy 2": dict(strategy=2),
    "strategy -1": dict(strategy=-1),
}


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_parameter_errors_come_back_before_the_device_is_touched(name, host):
    status, arrays, message = _call(_scene(), host, **ERRORS[name])
    assert status == RT_ERR_INVALID, message
    assert _names_no_device(message), message
    assert message.startswith(NAMES[1] if host else NAMES[0]), "the message names the call that refused"
    assert _untouched(arrays), "nothing was written"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_the_refusals_come_in_the_headers_order(host):
    """rt_scene_radiance's own, in its order, then the strategy."""
    order = [("count", dict(count=-1)), ("samples", dict(samples=0)), ("max_depth", dict(max_depth=-1)), ("variant", dict(variant=2)),
             ("origin", dict(origin=False)), ("output", dict(outputs=())), ("strategy", dict(strategy=5))]
    for k, (word, _) in enumerate(order):
        kw = {}
        for _, later in order[k:]:
            kw.update(later)
        status, _, message = _call(_scene(), host, **kw)
        assert status == RT_ERR_INVALID and word in message, (word, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_valid_parameters_get_as_far_as_the_device(host):
    """The other side of the table: the limits themselves are accepted (the call then fails on device ordinal 12345)."""
    for kw in (dict(), dict(samples=1 << 20), dict(max_depth=0), dict(variant=1), dict(count=1 << 30), dict(outputs=("path_rays",)),
               dict(strategy=0)):
        status, _, message = _call(_scene(), host, **kw)
        assert status != RT_OK and not _names_no_device(message), (kw, message)


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_a_query_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    status, _, message = _call(_scene(commit=False), host, strategy=7)   # the order of include/rtow.h: the state first
    assert status == RT_ERR_STATE, message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_empty_batch_is_ok_without_a_launch(host):
    status, arrays, message = _call(_scene(), host, count=0)
    assert status == RT_OK, message
    assert _untouched(arrays)
    status, _, message = _call(_scene(), host, count=0, origin=False, direction=False)   # no rays: no arrays needed
    assert status == RT_OK, message
    for kw in (dict(samples=0), dict(max_depth=-1), dict(variant=3), dict(outputs=()), dict(strategy=2)):   # ... the parameters are still checked
        status, _, _ = _call(_scene(), host, count=0, **kw)
        assert status == RT_ERR_INVALID, kw


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_radiance_direct_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.RadianceDirectParams, _lib.RadianceRays, _lib.RadianceOut, _lib.RadianceDirectStats)]
    assert list(sizes) == ours
    assert ours == [88, 32, 24, 40]   # rt_radiance_params' 72 + 4 x 4; the plain call's rays and outputs; 3 x 8 + 8 + 2 x 4
    plain = _lib.RadianceParams._fields_
    assert _lib.RadianceDirectParams._fields_[:len(plain)] == plain, "rt_radiance_params field for field"
    assert [name for name, _ in _lib.RadianceDirectParams._fields_[len(plain):]] == ["strategy", "reserved2"]
    for name, _ in plain:
        assert getattr(_lib.RadianceDirectParams, name).offset == getattr(_lib.RadianceParams, name).offset, name
    assert [name for name, _ in _lib.RadianceDirectStats._fields_] == ["rays", "shadow_rays", "shadow_reached", "seconds", "kernel_vgprs",
                                                                        "scratch_bytes"]
    plain_sizes = (C.c_uint32 * 4)()
    api.lib().rt_radiance_abi_sizes(plain_sizes)
    assert list(plain_sizes) == [72, 32, 24, 24], "no existing structure changed"


def test_direct_is_none_or_mis():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    for value in ("nee", "MIS", True, 1, ""):
        with pytest.raises(rt.RtowError) as info:
            s.radiance(o, d, device=12345, direct=value)
        assert "direct" in str(info.value) and "device" not in str(info.value), (value, str(info.value))
    for strategy in (2, -1, None):
        with pytest.raises(rt.RtowError) as info:
            s.radiance(o, d, device=12345, direct="mis", strategy=strategy)
        assert "strategy" in str(info.value) and "device" not in str(info.value), (strategy, str(info.value))
    for kw in (dict(direct=None), dict(direct=None, strategy=9), dict(direct="mis"), dict(direct="mis", strategy=0)):   # accepted: as far as the device
        with pytest.raises(rt.RtowError) as info:
            s.radiance(o, d, device=12345, **kw)
        assert "device" in str(info.value) or "HIP" in str(info.value), (kw, str(info.value))


def test_python_reports_the_librarys_errors():
    s = _scene()
    o, d = np.zeros((2, 3)), np.tile([0.0, 0.0, -1.0], (2, 1))
    for kw in (dict(samples=0), dict(samples=(1 << 20) + 1), dict(max_depth=-1), dict(variant=2)):
        with pytest.raises(rt.RtowError) as info:
            s.radiance(o, d, device=12345, direct="mis", **kw)
        assert "status 1" in str(info.value) and "rt_scene_radiance_direct:" in str(info.value), (kw, str(info.value))
    with pytest.raises(rt.RtowError) as info:
        _scene(commit=False).radiance(o, d, device=12345, direct="mis")
    assert "status 5" in str(info.value)
    with pytest.raises(rt.RtowError):   # the engine's refusals hold for the new call too
        s.radiance(o.astype(np.float32), d, device=12345, direct="mis")
    with pytest.raises(rt.RtowError):
        s.radiance(o, d, device=12345, direct="mis", samples=1.5)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    out = s.radiance(np.zeros((0, 3)), np.zeros((0, 3)), want=OUTPUTS, direct="mis")
    assert sorted(out) == sorted(OUTPUTS)
    assert out["radiance"].shape == (0, 3) and out["path_rays"].shape == (0,) and out["rng_state"].shape == (0, 6)
    out, st = s.radiance(np.zeros((0, 3)), np.zeros((0, 3)), stats=True, direct="mis", strategy=0)
    assert isinstance(st, _lib.RadianceDirectStats)
    assert list(out) == ["radiance"] and st.rays == 0 and st.shadow_rays == 0 and st.shadow_reached == 0 and st.seconds == 0.0
