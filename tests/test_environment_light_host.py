"""The environment as a light of the direct estimators, without a device (rt_scene_set_environment_light; include/rtow.h): what the
setter refuses and in which order, the getter before and after commit, the table of effective shares in all its rows through
``Scene.flags`` and ``Scene.environment_light``, and everything the bit must leave alone -- the light table, the scene's info, the
plan of a plain launch, the refusals of the three direct calls (the film's behind its NULL film only where a device is: a film
cannot exist without one) -- and the executable's option."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import test_film_direct_host as film_host
import test_path_advance_direct_host as advance_host
import test_radiance_direct_host as radiance_host
from conftest import ROOT
from frame_helpers import render_params

RT_OK, RT_ERR_INVALID = 0, 1
BIT = rt.SCENE_FLAG_ENVIRONMENT_LIGHT


def scene_of(lamps, environment=True, chance=None, commit=True):
    """A diffuse ball over a ground, with or without a lamp, with or without a sky; ``chance``: None never calls the setter."""
    s = rt.Scene()
    grey = s.Lambertian((0.5, 0.5, 0.5))
    items = [s.Sphere((0, -100.5, -3), 100.0, grey), s.Sphere((0, 0, -3), 0.5, grey)]
    if lamps:
        items.append(s.Quad((-1, 2, -4), (2, 0, 0), (0, 0, 2), s.DiffuseLight((4, 4, 4))))
    s.SetWorld(s.HittableList(items))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 1.0, 0.0, 1.0, background=(0, 0, 0))
    if environment:
        s.Environment(image=np.random.default_rng(1).uniform(0.05, 2.0, size=(4, 8, 3)).astype(np.float32))
    if chance is not None:
        s.EnvironmentLight(chance)
    if commit:
        s.Commit()
    return s


def test_the_header_names_the_bit_and_the_binding_has_the_calls():
    assert BIT == 2048 and "#define RT_SCENE_FLAG_ENVIRONMENT_LIGHT 2048u" in open(os.path.join(ROOT, "include", "rtow.h")).read()
    assert rt.lib().rt_scene_set_environment_light and rt.lib().rt_scene_get_environment_light


@pytest.mark.parametrize("chance", [float("nan"), -0.25, -1e-300, 1.0 + 2.0 ** -52, 2.0, float("inf"), -float("inf")])
def test_a_chance_outside_0_1_is_refused(chance):
    s = scene_of(True, chance=0.25)
    with pytest.raises(rt.RtowError, match=r"chance must lie in \[0, 1\]"):
        s.EnvironmentLight(chance)
    assert s.environment_light() == {"chance": 0.25, "effective": 0.25}, "a refused call changes nothing: the scene is still committed"


def test_the_refusals_come_in_the_headers_order():
    """The NULL scene before the chance (the state between them needs a render in flight: tests/test_environment_light_gpu.py)."""
    L = rt.lib()
    assert L.rt_scene_set_environment_light(None, C.c_double(float("nan"))) == RT_ERR_INVALID and b"null scene" in L.rt_last_error()
    assert L.rt_scene_set_environment_light(None, C.c_double(0.5)) == RT_ERR_INVALID and b"null scene" in L.rt_last_error()
    assert L.rt_scene_get_environment_light(None, None, None) == RT_ERR_INVALID and b"null scene" in L.rt_last_error()
    s = scene_of(True, commit=False)
    for ok in (0.0, 1.0, 0.5, 5e-324):
        s.EnvironmentLight(ok)
    assert L.rt_scene_get_environment_light(s._p, None, None) == RT_OK, "either pointer may be NULL"


def test_the_getter_before_and_after_commit_and_the_call_uncommits():
    s = scene_of(True, commit=False)
    assert s.environment_light() == {"chance": 0.0, "effective": 0.0}, "the default"
    s.EnvironmentLight()
    assert s.environment_light() == {"chance": 0.5, "effective": 0.0}, "effective is 0 before commit"
    s.Commit()
    assert s.environment_light() == {"chance": 0.5, "effective": 0.5} and s.flags() & BIT
    s.EnvironmentLight(0.75)   # a construction call: the scene counts as not committed behind it
    with pytest.raises(rt.RtowError, match="not committed"):
        s.info()
    assert s.environment_light() == {"chance": 0.75, "effective": 0.0} and s.flags() == 0
    s.Commit()
    assert s.environment_light() == {"chance": 0.75, "effective": 0.75}
    assert "chance" not in (s.environment() or {}) and "effective" not in s.environment(), "Scene.environment() keeps its keys"


@pytest.mark.parametrize("lamps,environment,chance,c_e,bit", [
    (True, False, 0.5, 0.0, False), (False, False, 1.0, 0.0, False),       # no environment
    (True, True, 0.0, 0.0, False), (False, True, 0.0, 0.0, False),         # chance == 0
    (False, True, 0.5, 1.0, True), (False, True, 1e-9, 1.0, True),         # environment, chance > 0, no lights
    (True, True, 0.5, 0.5, True), (True, True, 0.3, 0.3, True), (True, True, 1.0, 1.0, True),   # environment, chance > 0, lights
])
def test_the_table_of_effective_shares(lamps, environment, chance, c_e, bit):
    s = scene_of(lamps, environment, chance)
    never = scene_of(lamps, environment, None)
    assert s.info()["n_lights"] == (1 if lamps else 0)
    assert s.environment_light() == {"chance": chance, "effective": c_e}
    assert bool(s.flags() & BIT) == bit
    assert s.flags() & ~BIT == never.flags(), "no other bit moves"
    if not bit:
        assert s.flags() == never.flags(), "chance 0, or no environment: the flags word of a scene that never called the setter"


def test_the_chance_survives_a_change_of_environment_and_waits_for_one():
    s = scene_of(True, environment=False, chance=0.25)
    assert s.flags() & BIT == 0 and s.environment_light() == {"chance": 0.25, "effective": 0.0}
    s.Environment(texture=s.SolidColor((0.5, 0.7, 1.0)))
    s.Commit()
    assert s.flags() & BIT and s.environment_light() == {"chance": 0.25, "effective": 0.25}
    s.Environment(image=np.ones((2, 2, 3), dtype=np.float32))
    s.Commit()
    assert s.flags() & BIT and s.environment_light()["effective"] == 0.25
    s.Environment()
    s.Commit()
    assert s.flags() & BIT == 0 and s.environment_light() == {"chance": 0.25, "effective": 0.0}


@pytest.mark.parametrize("lamps", [False, True])
def test_the_light_table_the_info_and_the_plain_plan_do_not_see_the_bit(lamps):
    off, on = scene_of(lamps, chance=None), scene_of(lamps, chance=0.5)
    assert on.flags() == off.flags() | BIT
    a, b = off.lights(), on.lights()
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), "rt_scene_dump_lights: the environment is no row"
    assert on.info() == off.info()
    p = render_params(16, 16, 4)
    for adaptive in (False, True):
        assert on.plan_launch(p, adaptive=adaptive) == off.plan_launch(p, adaptive=adaptive), "choose_kernel and the plans do not react"


@pytest.mark.parametrize("host", [True, False], ids=["host", "device"])
def test_the_direct_calls_refuse_what_they_refused(host):
    """The refusal tables of tests/test_path_advance_direct_host.py and tests/test_radiance_direct_host.py, on a scene with the bit."""
    scene = scene_of(True, chance=0.5)
    for name, kw in sorted(advance_host.ERRORS.items()):
        status, arrays, message = advance_host._call(scene, host, **kw)
        advance_host._is_parameter_error(status, arrays, message, host)
    for name, kw in sorted(radiance_host.ERRORS.items()):
        status, arrays, message = radiance_host._call(scene, host, **kw)
        assert status == RT_ERR_INVALID and radiance_host._names_no_device(message) and radiance_host._untouched(arrays), (name, message)
    for module in (advance_host, radiance_host):   # ... and valid parameters still get as far as the device
        status, _, message = module._call(scene, host)
        assert status != RT_OK and ("device" in message or "HIP" in message), message
    fresh = scene_of(True, chance=0.5, commit=False)
    assert advance_host._call(fresh, host)[0] == advance_host.RT_ERR_STATE and radiance_host._call(fresh, host)[0] == radiance_host.RT_ERR_STATE


def test_the_direct_film_refuses_a_null_film_first_whatever_direct_holds():
    """tests/test_film_direct_host.py's refusal that needs no device, on a scene with the bit."""
    from raytracinginoneweekendincuda_amd import _lib
    scene = scene_of(True, chance=0.5)
    assert scene.flags() & BIT
    for direct in (None, _lib.FilmDirectParams(2), _lib.FilmDirectParams(1)):
        assert abs(film_host._launch(scene, None, film_host._params(), direct)) == RT_ERR_INVALID
        message = rt.lib().rt_last_error().decode()
        assert "rt_render_launch_direct" in message and "null" in message


def test_the_direct_film_refuses_what_it_refused():
    """The refusals of rt_render_launch_direct behind the NULL film, as tests/test_film_direct_host.py pins them, on a scene with the
    bit: strategy 2 and -1, a non-zero reserved word, a NULL direct, and the plain launch's geometry mismatch before all of them."""
    if not torch.cuda.is_available():
        pytest.skip("a film cannot exist without a device (rt_film_create selects it): these refusals run where one is")
    from raytracinginoneweekendincuda_amd import _lib
    for lamps in (True, False):
        scene = scene_of(lamps, chance=0.5)
        assert scene.flags() & BIT
        film = rt.Film(film_host.W, film_host.H)
        reserved = _lib.FilmDirectParams(1)
        reserved.reserved[6] = 1
        for direct, word in ((_lib.FilmDirectParams(2), "strategy"), (_lib.FilmDirectParams(-1), "strategy"), (reserved, "reserved"), (None, "direct")):
            assert abs(film_host._launch(scene, film, film_host._params(), direct)) == RT_ERR_INVALID
            assert word in rt.lib().rt_last_error().decode()
        assert abs(film_host._launch(scene, film, film_host._params(width=film_host.W + 1), _lib.FilmDirectParams(2))) == RT_ERR_INVALID
        assert "geometry" in rt.lib().rt_last_error().decode()
        with pytest.raises(rt.RtowError, match="no direct launch"):   # nothing was launched by any of them
            film.direct_stats()
        with pytest.raises(rt.RtowError, match="nothing launched"):
            film.finish(scene)


def test_the_params_structs_of_the_direct_calls_are_what_they_were():
    """The switch is a property of the scene: no field joined the three calls' structs."""
    from raytracinginoneweekendincuda_amd import _lib
    assert [n for n, _ in _lib.PathAdvanceDirectParams._fields_][-2:] == ["strategy", "sample"]
    assert [n for n, _ in _lib.RadianceDirectParams._fields_][-2:] == ["strategy", "reserved2"]
    assert [n for n, _ in _lib.FilmDirectParams._fields_] == ["strategy", "reserved"]


def run_rtow(*options):
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    return subprocess.run([exe, *options, "--width", "16", "--height", "16", "--spp", "1"], cwd=ROOT, timeout=120, capture_output=True, text=True)


def test_rtow_refuses_environment_light_without_direct_mis():
    """Refused while the options are read: no scene is built, no device is touched."""
    run = run_rtow("--scene", "15", "--environment-light", "0.5")
    assert run.returncode == 2 and "--environment-light goes with --direct mis" in run.stderr
    run = run_rtow("--scene", "15", "--environment-light", "0.5", "--radiance-at", "3,3")
    assert run.returncode == 2 and "--direct mis" in run.stderr
    for bad in ("1.5", "nan"):
        run = run_rtow("--scene", "15", "--direct", "mis", "--environment-light", bad, "--radiance-at", "3,3")
        assert run.returncode == 2 and "[0, 1]" in run.stderr, (bad, run.stderr)
    for bad in ("abc", "0.5x", ""):   # not a number: refused, not read as 0 (which would switch the feature off without a word)
        run = run_rtow("--scene", "15", "--direct", "mis", "--environment-light", bad, "--radiance-at", "3,3")
        assert run.returncode == 2 and "needs a number" in run.stderr, (bad, run.stderr)


def test_rtow_refuses_environment_light_for_a_scene_without_an_environment():
    """Scene 10 has none: refused when the scene is built, on the host, before anything is rendered."""
    run = run_rtow("--scene", "10", "--direct", "mis", "--environment-light", "0.5", "--radiance-at", "3,3")
    assert run.returncode == 1 and "--environment-light: the scene has no environment" in run.stderr, run.stderr
