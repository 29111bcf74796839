"""Ray queries (include/rtow.h rt_scene_intersect): what can be checked without a device -- every parameter error comes back before
the device is touched, an empty batch is no launch, the ctypes structures have the library's sizes, and the Python layer refuses
arrays it would have to convert."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

INF = float("inf")
RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5


def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, -3), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _call(scene, host, count=1, tmin=0.001, tmax=INF, mode=0, variant=0, origin=True, direction=True, per_ray_tmin=None):
    """The raw C call with one ray (0, 0, 0) -> (0, 0, -1) repeated; returns (status, t array).  A device ordinal no machine has:
    a call that got as far as the device would say so (RT_ERR_NO_DEVICE or RT_ERR_INVALID 'device ordinal'), and the message
    of a parameter error never mentions the device."""
    n = max(count, 1) if count <= 4 else 1
    o = np.zeros((n, 3))
    d = np.tile([0.0, 0.0, -1.0], (n, 1))
    t = np.full(n, -1.0)
    p = _lib.QueryParams(count, tmin, tmax, 0.0, 1984, 0, mode, variant, 12345, None)
    rays = _lib.QueryRays(o.ctypes.data if origin else None, d.ctypes.data if direction else None, None,
                          per_ray_tmin.ctypes.data if per_ray_tmin is not None else None, None)
    hits = _lib.QueryHits(t=t.ctypes.data)
    fn = api.lib().rt_scene_intersect if host else api.lib().rt_scene_intersect_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(hits), None)
    return status, t, api.lib().rt_last_error().decode()


ERRORS = {
    "negative count": (dict(count=-1), RT_ERR_INVALID),
    "count above 2^30": (dict(count=(1 << 30) + 1), RT_ERR_INVALID),
    "null origin": (dict(origin=False), RT_ERR_INVALID),
    "null direction": (dict(direction=False), RT_ERR_INVALID),
    "mode 2": (dict(mode=2), RT_ERR_INVALID),
    "mode -1": (dict(mode=-1), RT_ERR_INVALID),
    "variant 2": (dict(variant=2), RT_ERR_INVALID),
    "tmin NaN": (dict(tmin=float("nan")), RT_ERR_INVALID),
    "tmax below tmin": (dict(tmin=2.0, tmax=1.0), RT_ERR_INVALID),
    "tmax NaN": (dict(tmax=float("nan")), RT_ERR_INVALID),
}


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(ERRORS))
def test_parameter_errors_come_back_before_the_device_is_touched(name, host):
    kw, want = ERRORS[name]
    status, t, message = _call(_scene(), host, **kw)
    assert status == want, message
    assert "device" not in message.replace("rt_scene_intersect_device", "") and "HIP" not in message, message
    assert (t == -1.0).all(), "nothing was written"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_a_query_before_commit_is_a_state_error(host):
    status, _, message = _call(_scene(commit=False), host)
    assert status == RT_ERR_STATE, message
    status, _, message = _call(_scene(commit=False), host, mode=7)   # the order of include/rtow.h: the state first
    assert status == RT_ERR_STATE, message


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_an_empty_batch_is_ok_without_a_launch(host):
    status, t, message = _call(_scene(), host, count=0)
    assert status == RT_OK, message
    assert (t == -1.0).all()
    status, _, message = _call(_scene(), host, count=0, origin=False, direction=False)   # no rays: no arrays needed
    assert status == RT_OK, message
    status, _, _ = _call(_scene(), host, count=0, mode=3)   # ... but the parameters are still checked
    assert status == RT_ERR_INVALID


def test_the_scalar_interval_is_not_checked_where_per_ray_arrays_replace_it():
    """tmin = NaN in the parameters means nothing when rays->tmin is given: the call then gets as far as the device (ordinal 12345)."""
    status, _, message = _call(_scene(), True, tmin=float("nan"), per_ray_tmin=np.full(1, 0.001))
    assert status != RT_OK and ("device" in message or "HIP" in message), message


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 4)()
    api.lib().rt_query_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.QueryParams, _lib.QueryRays, _lib.QueryHits, _lib.QueryStats)]
    assert list(sizes) == ours
    assert ours == [88, 40, 64, 32]   # include/rtow.h on LP64: 8 + 4 x 8 + 8 + 3 x 4 (+ 4 pad) + 8 + 16; 5 and 8 pointers; 2 x 8 + 8 + 2 x 4
    assert [name for name, _ in _lib.QueryHits._fields_] == ["t", "normal", "uv", "albedo", "leaf", "front_face", "material", "occluded"]


def test_python_refuses_arrays_it_would_have_to_convert():
    s = _scene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, -1.0], (4, 1))
    cases = {
        "float32 origins": (o.astype(np.float32), d, {}),
        "float32 directions": (o, d.astype(np.float32), {}),
        "strided origins": (np.zeros((4, 6))[:, ::2], d, {}),
        "strided directions": (o, np.asfortranarray(d), {}),
        "a list": (o.tolist(), d, {}),
        "wrong trailing shape": (np.zeros((4, 2)), d, {}),
        "counts differ": (o, d[:3].copy(), {}),
        "float32 times": (o, d, dict(times=np.zeros(4, dtype=np.float32))),
        "strided tmin": (o, d, dict(tmin=np.zeros(8)[::2])),
        "tmax of another length": (o, d, dict(tmax=np.ones(5))),
        "unknown output": (o, d, dict(want=("t", "colour"))),
    }
    for name, (origins, directions, kw) in cases.items():
        for call in (s.intersect, s.occluded):
            if "want" in kw and call == s.occluded:
                continue
            with pytest.raises(rt.RtowError):
                call(origins, directions, **kw)
                pytest.fail(name + " was accepted")
    assert np.zeros((4, 6))[:, ::2].shape == (4, 3) and not np.asfortranarray(d).flags.c_contiguous   # (the cases are what they say)


def test_python_passes_an_empty_batch_through():
    s = _scene()
    out = s.intersect(np.zeros((0, 3)), np.zeros((0, 3)))
    assert sorted(out) == sorted(("t", "normal", "uv", "albedo", "leaf", "front_face", "material"))
    assert out["t"].shape == (0,) and out["normal"].shape == (0, 3) and out["uv"].shape == (0, 2) and out["leaf"].dtype == np.int32
    hit, st = s.occluded(np.zeros((0, 3)), np.zeros((0, 3)), stats=True)
    assert hit.shape == (0,) and hit.dtype == bool and st.rays == 0 and st.hits == 0
