"""Light sampling queries (include/rtow.h rt_scene_dump_lights, rt_scene_sample_lights, rt_scene_light_pdf): what can be checked
without a device -- the light table of constructed worlds and of the built-in scenes, the refusals in their order, the sizes of the
ctypes structures, and the numpy restatement (tests/light_restated.py) against closed forms."""
import ctypes as C
import math

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api

import light_restated as lr
from light_worlds import mixed_world, no_lights_world

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, 1, 5
GUARD = 0xAB


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the light table ----
def test_light_table_of_a_constructed_world():
    s, expected, _ = mixed_world()
    L = s.lights()
    assert s.info()["n_lights"] == len(expected) == len(L["kind"]) == 13
    kinds, _ = s.dump_leaves()
    for k, (kind, leaf, mat, fields) in enumerate(expected):
        assert (L["kind"][k], L["leaf"][k], L["material"][k]) == (kind, leaf, mat), k
        assert 0 <= leaf < len(kinds)
        for name, want in fields.items():
            assert np.array_equal(L[name][k], np.asarray(want, dtype=np.float64)), (k, name, L[name][k], want)
    assert abs(L["s"][1] - 0.5 * math.sqrt(0.25 + 0.0625 + 1.0)) < 1e-15   # the triangle's area
    assert np.all(np.abs(np.sqrt((L["n"][L["kind"] <= 1] ** 2).sum(axis=1)) - 1.0) < 1e-15)   # unit normals


def test_transformed_quad_is_the_restated_transform_bit_for_bit():
    s, expected, _ = mixed_world()
    L = s.lights()
    k = [i for i, e in enumerate(expected) if "n" in e[3]][0]
    f = expected[k][3]
    for name in ("a", "b", "c", "n"):
        assert np.array_equal(_bits(L[name][k]), _bits(f[name])), name
    # ... and so are its corners Q, Q + u, Q + v
    got = np.stack([L["a"][k], L["a"][k] + L["b"][k], L["a"][k] + L["c"][k]])
    want = np.stack([f["a"], f["a"] + f["b"], f["a"] + f["c"]])
    assert np.array_equal(_bits(got), _bits(want))


def test_cumulative_tables():
    s, expected, emission = mixed_world()
    L = s.lights()
    n = len(expected)
    for st in (0, 1):
        cdf = L["cdf"][:, st]
        assert np.all(np.diff(cdf) >= 0.0) and cdf[0] > 0.0 and cdf[-1] == 1.0
    assert np.array_equal(L["cdf"][:-1, 0], np.arange(1, n) / float(n))
    # strategy 1: area x the brightest channel of a solid emitter, x 1 of a checker
    area = np.where(L["kind"] >= 2, 4.0 * lr.PI * (L["s"] * L["s"]), L["s"])
    bright = np.array([max(emission[m][1]) if emission[m][0] == "solid" else 1.0 for m in L["material"]])
    w = area * bright
    run, want = 0.0, []
    for x in w:
        run += x
        want.append(run)
    want = np.array(want) / run
    want[-1] = 1.0
    assert np.array_equal(L["cdf"][:, 1], want)


def test_builtin_scenes_report_their_lamps():
    for scene_id, lamp in ((7, ((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0))),
                           (9, ((123.0, 554.0, 147.0), (300.0, 0.0, 0.0), (0.0, 0.0, 265.0)))):
        s = rt.builtin_scene(scene_id, 0, 32, 32)
        L = s.lights()
        assert s.info()["n_lights"] == 1 and list(L["kind"]) == [0]
        assert np.array_equal(np.stack([L["a"][0], L["b"][0], L["c"][0]]), np.array(lamp))
        kinds, boxes = s.dump_leaves()
        assert kinds[L["leaf"][0]] == 2 and boxes[L["leaf"][0]][2] <= 554.0 <= boxes[L["leaf"][0]][3]
        assert L["cdf"].tolist() == [[1.0, 1.0]]
    s = rt.builtin_scene(1, 0, 32, 32)
    assert s.info()["n_lights"] == 0 and len(s.lights()["kind"]) == 0 and s.lights()["cdf"].shape == (0, 2)
    assert no_lights_world().info()["n_lights"] == 0


def test_the_executable_lists_the_lights():
    """rtow --lights: the table of rt_scene_dump_lights, a line per light, no render and no device."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    run = subprocess.run([exe, "--scene", "7", "--lights"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[0] == "1 lights" and len(lines) == 2
    words = lines[1].split()
    assert words[:6] == ["0", "quad", "leaf", "6", "material", "3"]
    at = {w: k for k, w in enumerate(words)}
    assert [float(x) for x in words[at["Q"] + 1:at["Q"] + 4]] == [343.0, 554.0, 332.0] and float(words[at["area"] + 1]) == 13650.0
    assert [float(x) for x in words[at["cdf"] + 1:]] == [1.0, 1.0]
    none = subprocess.run([exe, "--scene", "1", "--lights"], capture_output=True, text=True, timeout=60)
    assert none.returncode == 0 and none.stdout.strip() == "0 lights"


def test_a_graph_too_deep_for_the_light_walk_is_refused():
    s = rt.Scene()
    obj = s.Sphere((0, 0, 0), 1.0, s.DiffuseLight((1, 1, 1)))
    for _ in range(70):
        obj = s.Translate(obj, (0.1, 0, 0))
    s.SetWorld(s.HittableList([obj]))
    s.Camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40, 1.0, 0.0, 10.0)
    with pytest.raises(rt.RtowError, match="nesting deeper"):
        s.Commit()


# ---- refusals ----
def _scene(commit=True):
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), s.DiffuseLight((4, 4, 4)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    if commit:
        s.Commit()
    return s


def _sample(scene, host, count=1, strategy=0, variant=0, point=True, outputs=tuple(_lib.LIGHT_SAMPLE_OUTPUTS), normal=True, material=True):
    n = 1
    pt, nm, mt = np.zeros((n, 3)), np.tile([0.0, 1.0, 0.0], (n, 1)), np.zeros(n, dtype=np.uint8)
    arrays = {name: np.full(n * int(np.prod(tail, dtype=np.int64)) * np.dtype(dtype).itemsize, GUARD, dtype=np.uint8)
              for name, (dtype, tail) in _lib.LIGHT_SAMPLE_OUTPUTS.items()}
    p = _lib.LightParams(count, 0.0, 1984, 0, strategy, variant, 12345, None)   # a device ordinal no machine has
    pts = _lib.LightPoints(pt.ctypes.data if point else None, nm.ctypes.data if normal else None, mt.ctypes.data if material else None, None, None)
    out = _lib.LightSamples(**{name: arrays[name].ctypes.data for name in outputs})
    fn = api.lib().rt_scene_sample_lights if host else api.lib().rt_scene_sample_lights_device
    status = fn(scene._p, C.byref(p), C.byref(pts), C.byref(out), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _pdf(scene, host, count=1, strategy=0, variant=0, origin=True, direction=True, outputs=("pdf", "light")):
    o, d = np.zeros((1, 3)), np.tile([0.0, 1.0, 0.0], (1, 1))
    arrays = {"pdf": np.full(8, GUARD, dtype=np.uint8), "light": np.full(4, GUARD, dtype=np.uint8)}
    p = _lib.LightParams(count, 0.0, 0, 0, strategy, variant, 12345, None)
    rays = _lib.LightRays(o.ctypes.data if origin else None, d.ctypes.data if direction else None, None)
    out = _lib.LightPdfOut(**{name: arrays[name].ctypes.data for name in outputs})
    fn = api.lib().rt_scene_light_pdf if host else api.lib().rt_scene_light_pdf_device
    status = fn(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    return status, arrays, api.lib().rt_last_error().decode()


def _names_the_device(message):
    """The call got as far as the device, which ordinal 12345 is not."""
    for name in ("rt_scene_sample_lights_device", "rt_scene_light_pdf_device"):
        message = message.replace(name, "")
    return "device" in message or "HIP" in message


# the refusal table of include/rtow.h, in its order: each entry also carries every fault that comes after it in the table, and the
# message must name the first
SAMPLE_ERRORS = [("count", dict(count=-1)), ("count", dict(count=(1 << 30) + 1)), ("strategy", dict(strategy=2)), ("strategy", dict(strategy=-1)),
                 ("variant", dict(variant=2)), ("null point", dict(point=False)), ("every output is null", dict(outputs=())),
                 ("need normal and material", dict(normal=False)), ("need normal and material", dict(material=False))]
PDF_ERRORS = [("count", dict(count=-1)), ("strategy", dict(strategy=2)), ("variant", dict(variant=-1)), ("null origin or direction", dict(origin=False)),
              ("null origin or direction", dict(direction=False)), ("every output is null", dict(outputs=()))]


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
@pytest.mark.parametrize("call, errors", [(_sample, SAMPLE_ERRORS), (_pdf, PDF_ERRORS)], ids=["sample", "pdf"])
def test_refusals_in_order_before_the_device_is_touched(call, errors, host):
    s = _scene()
    for k, (word, kw) in enumerate(errors):
        later = {}
        for _, other in errors[k:]:
            later = {**other, **later}   # this fault and every later one at once (the earliest setting of a parameter wins)
        status, arrays, message = call(s, host, **later)
        assert status == RT_ERR_INVALID and word in message, (word, later, message)
        assert "HIP" not in message and all((a == GUARD).all() for a in arrays.values()), message
    status, _, message = call(_scene(commit=False), host, count=-1)   # the state comes first
    assert status == RT_ERR_STATE, message
    # the other side: valid parameters get as far as the device, and an empty batch is no launch
    status, _, message = call(s, host)
    assert status != RT_OK and _names_the_device(message), message
    status, arrays, message = call(s, host, count=0)
    assert status == RT_OK and all((a == GUARD).all() for a in arrays.values()), message
    status, _, _ = call(s, host, count=0, strategy=3)
    assert status == RT_ERR_INVALID


def test_scatter_outputs_alone_need_normal_and_material():
    s = _scene()
    for name in ("scatter_pdf", "contribution"):
        status, _, message = _sample(s, True, outputs=(name,), normal=False)
        assert status == RT_ERR_INVALID and "normal and material" in message
    status, _, message = _sample(s, True, outputs=("pdf",), normal=False, material=False)
    assert status != RT_OK and _names_the_device(message), message   # without them the other outputs are served


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 8)()
    api.lib().rt_light_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (_lib.LightParams, _lib.LightPoints, _lib.LightSamples, _lib.LightRays, _lib.LightPdfOut, _lib.LightStats, _lib.LightRow)]
    assert list(sizes)[:7] == ours == [72, 40, 64, 24, 16, 32, 128]
    assert sizes[7] == _lib.light_lds_rows() and sizes[7] % 2 == 0
    assert 4 * sizes[7] * (128 + 8) <= 160 * 1024   # four workgroups' staged rows and table entries fit a CU's LDS
    assert [n for n, _ in _lib.LightSamples._fields_] == list(_lib.LIGHT_SAMPLE_OUTPUTS)
    assert [n for n, _ in _lib.LightPoints._fields_] == ["point", "normal", "material", "time", "rng_state"]


def test_shadow_rays_rule():
    p, d, dist = np.zeros((2, 3)), np.tile([0.0, 1.0, 0.0], (2, 1)), np.array([2.0, 1e6])
    o, dd, times, tmin, tmax = rt.Scene.shadow_rays(p, d, dist)
    assert o is p and dd is d and times is None and tmin == 0.001
    assert np.array_equal(tmax, dist * (1.0 - 2.0 ** -20)) and np.all(tmax < dist)


# ---- the restatement against closed forms ----
def _one_light(kind, **fields):
    L = {name: np.zeros((1, 3)) for name in ("a", "b", "c", "n")}
    L.update(s=np.zeros(1), kind=np.array([kind], dtype=np.int32), leaf=np.zeros(1, dtype=np.int32), material=np.zeros(1, dtype=np.int32),
             cdf=np.ones((1, 2)))
    for name, v in fields.items():
        L[name][0] = v
    return L


def _join(*tables):
    L = {name: np.concatenate([t[name] for t in tables]) for name in tables[0] if name != "cdf"}
    n = len(tables)
    L["cdf"] = np.tile((np.arange(1, n + 1) / float(n))[:, None], (1, 2))
    L["cdf"][-1] = 1.0
    return L


def _rectangle_solid_angle(x0, x1, y0, y1, h):
    """Of the rectangle [x0, x1] x [y0, y1] in the plane at height h above the eye (the arctangent closed form)."""
    def corner(x, y):
        return math.atan(x * y / (h * math.sqrt(x * x + y * y + h * h)))
    return corner(x1, y1) - corner(x0, y1) - corner(x1, y0) + corner(x0, y0)


def test_restated_quad_samples_integrate_to_the_solid_angle():
    n = 20000
    L = _one_light(lr.QUAD, a=(-0.5, 2.0, -1.0), b=(2.0, 0.0, 0.0), c=(0.0, 0.0, 1.5), n=(0.0, 1.0, 0.0), s=3.0)
    P = np.tile([0.25, 0.5, 0.1], (n, 1))
    out = lr.sample_lights(L, P, lr.seeded_states(n, seed=11), emission=None)
    assert out["valid"].all()
    x = 1.0 / out["pdf"]
    want = _rectangle_solid_angle(-0.75, 1.25, -1.1, 0.4, 1.5)
    se = x.std(ddof=1) / math.sqrt(n)
    assert abs(x.mean() - want) <= 5.0 * se and se < 0.01 * want, (x.mean(), want, se)
    # the samples lie on the quad, along the direction, at the distance
    S = P + out["distance"][:, None] * out["direction"]
    assert np.all(np.abs(S[:, 1] - 2.0) < 1e-14) and np.all((S[:, 0] > -0.5 - 1e-14) & (S[:, 0] < 1.5 + 1e-14))
    assert np.all(np.abs(np.sqrt((out["direction"] ** 2).sum(axis=1)) - 1.0) < 1e-15)


def test_restated_triangle_samples_integrate_to_half_the_quads_solid_angle_sum():
    """A quad cut along its diagonal into two triangles (Q, u, v) and (Q + u + v, -u, -v): under strategy 0 the mean of 1 / pdf over
    samples of the pair is the quad's solid angle."""
    n = 20000
    q, u, v = np.array([-0.5, 2.0, -1.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.5])
    L = _join(_one_light(lr.TRIANGLE, a=q, b=u, c=v, n=(0.0, 1.0, 0.0), s=1.5), _one_light(lr.TRIANGLE, a=q + u + v, b=-u, c=-v, n=(0.0, 1.0, 0.0), s=1.5))
    P = np.tile([0.25, 0.5, 0.1], (n, 1))
    out = lr.sample_lights(L, P, lr.seeded_states(n, seed=12))
    x = 1.0 / out["pdf"]
    want = _rectangle_solid_angle(-0.75, 1.25, -1.1, 0.4, 1.5)
    se = x.std(ddof=1) / math.sqrt(n)
    assert abs(x.mean() - want) <= 5.0 * se and se < 0.01 * want, (x.mean(), want, se)
    assert set(out["light"]) == {0, 1}


def test_restated_sphere_samples_integrate_to_the_caps():
    """Two spheres of different sizes under strategy 0: 1 / pdf is twice the picked sphere's cap, so the mean is the sum of the two
    caps, 2 pi (1 - cosmax) each -- evaluated here as 2 pi (r^2 / d^2) / (1 + cosmax), which does not cancel."""
    n = 20000
    L = _join(_one_light(lr.SPHERE, a=(0.0, 3.0, 0.0), s=0.5), _one_light(lr.MSPHERE, a=(2.0, 1.0, 1.0), b=(1.0, 0.0, 0.0), c=(0.0, 2.0, 0.0), s=1.0))
    P = np.tile([0.25, -0.5, 0.1], (n, 1))
    out = lr.sample_lights(L, P, lr.seeded_states(n, seed=13), time=1.0)
    assert out["valid"].all()
    want = 0.0
    for c, r in (((0.0, 3.0, 0.0), 0.5), ((2.5, 1.0, 1.0), 1.0)):   # the moving sphere at time 1 of [0, 2]
        d2 = sum((a - b) ** 2 for a, b in zip(c, (0.25, -0.5, 0.1)))
        want += 2.0 * math.pi * (r * r / d2) / (1.0 + math.sqrt(1.0 - r * r / d2))
    x = 1.0 / out["pdf"]
    se = x.std(ddof=1) / math.sqrt(n)
    assert se > 0.0 and abs(x.mean() - want) <= 5.0 * se and se < 0.01 * want, (x.mean(), want, se)
    # every sample lies on its sphere, on the near side, inside the cone
    C = np.where((out["light"] == 0)[:, None], np.array([0.0, 3.0, 0.0]), np.array([2.5, 1.0, 1.0]))
    r = np.where(out["light"] == 0, 0.5, 1.0)
    S = P + out["distance"][:, None] * out["direction"]
    assert np.all(np.abs(np.sqrt(((S - C) ** 2).sum(axis=1)) - r) < 1e-12)
    assert np.all(((S - C) * out["direction"]).sum(axis=1) <= 1e-12)
    # a point inside a sphere: an invalid sample, and the stream has moved on all the same
    inside = lr.sample_lights(_one_light(lr.SPHERE, a=(0.0, 0.0, 0.0), s=1.0), np.zeros((4, 3)) + 0.25, lr.seeded_states(4, seed=5))
    assert not inside["valid"].any() and np.all(inside["pdf"] == 0.0) and np.all(inside["light"] == 0)
    assert (inside["rng_state"] != lr.seeded_states(4, seed=5)).any(axis=1).all()


def test_restated_pdf_of_a_sampled_direction_is_the_sampled_pdf():
    s, _, emission = mixed_world()
    L = s.lights()
    n = 512
    P = np.tile([0.5, 0.25, 6.0], (n, 1)) + np.random.default_rng(3).uniform(-0.5, 0.5, size=(n, 3))
    out = lr.sample_lights(L, P, lr.seeded_states(n, seed=21), strategy=1, emission=emission, time=0.5)
    v = out["valid"]
    assert v.mean() > 0.9
    pdf, light = lr.light_pdf(L, P[v], out["direction"][v], strategy=1, time=0.5)
    # the mixture is at least the sampled light's own density, and equal where the ray meets no other light
    assert np.all(pdf >= out["pdf"][v] * (1.0 - 1e-9))
    alone = np.abs(pdf - out["pdf"][v]) <= 1e-9 * pdf
    assert alone.mean() > 0.5 and np.all((light >= 0))


def test_scatter_pdf_integrates_to_one():
    m = 200000
    theta = (np.arange(m) + 0.5) * (math.pi / m)
    d = np.stack([np.sin(theta), np.zeros(m), np.cos(theta)], axis=1)
    normals = np.tile([0.0, 0.0, 1.0], (m, 1))
    for kind, total in ((0, 1.0), (4, 1.0), (1, 0.0), (2, 0.0), (3, 0.0), (255, 0.0)):
        p = rt.scatter_pdf(np.full(m, kind, dtype=np.uint8), normals, d)
        got = float(np.sum(p * 2.0 * math.pi * np.sin(theta)) * (math.pi / m))
        assert abs(got - total) < 1e-8, (kind, got)
    # straight up it is twice a cosine lobe's 1 / pi
    assert rt.scatter_pdf(np.zeros(1, dtype=np.uint8), normals[:1], normals[:1])[0] == 2.0 / lr.PI
