"""Frames with light samples (rt_render_launch_direct), what can be checked without a GPU: the declarations and their bindings, the
structures' sizes, Rng.from_state, the restated camera rays, the refusals and the loud failure of a launch without a device.
A film cannot exist without a device (rt_film_create selects it), so on a machine without one the refusals that need a film are
shown as far as they can be reached -- the NULL film, which every launch refuses first; the test of the refusals behind it says
that it is skipped there, and runs wherever a device is; tests/test_film_direct_gpu.py runs them as well."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib

import film_direct_restated as fdr
from test_radiance_gpu import camera_rays, host_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_render_launch_direct", "rt_film_last_direct_stats", "rt_film_direct_abi_sizes", "rt_rng_create_from_state")
W, H = 20, 13
INVALID = 1   # RT_ERR_INVALID (include/rtow.h)


def test_the_header_declares_the_new_symbols_and_the_binding_has_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtow.h")).read(), flags=re.S)
    declared = set(re.findall(r"RTOW_API[^;(]*?\b(rt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(rt.lib(), name), name
    assert re.search(r"RT_ERR_INVALID\s*=\s*%d\b" % INVALID, text)


def test_ctypes_structures_have_the_librarys_sizes():
    sizes = (C.c_uint32 * 2)()
    rt.lib().rt_film_direct_abi_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.FilmDirectParams), C.sizeof(_lib.FilmDirectStats)] == [32, 24]


def test_rng_from_state_continues_the_stream():
    a = rt.Rng(1984, 7)
    for _ in range(5):
        a.uniform()
    state = a.state()
    b = rt.Rng.from_state(state)
    assert b.state() == state
    for _ in range(20):
        assert a.next_u32() == b.next_u32()
    c = rt.Rng.from_state(a.state())
    for _ in range(20):
        assert a.uniform() == c.uniform()
    assert a.state() == c.state()
    with pytest.raises(ValueError):
        rt.Rng.from_state([1, 2, 3])


def test_camera_rays_from_seeded_states_are_the_camera_rays():
    scene = rt.builtin_scene(7, 0, W, H)
    want = camera_rays(scene, seed=77, width=W, height=H)
    first = host_states(77, 0, W * H)
    assert np.array_equal(first, fdr.seeded_states(77, W, H))
    got = fdr.camera_rays_from(scene, first, W, H)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # ... and the second camera ray of a pixel continues where the first left the stream
    again = fdr.camera_rays_from(scene, got[3], W, H, pixels=[3, 41])
    assert np.array_equal(again[3][[0, 5]], got[3][[0, 5]]) and not np.array_equal(again[3][[3, 41]], got[3][[3, 41]])
    assert not np.array_equal(again[1][3], got[1][3]) and np.all(again[1][0] == 0.0)


def _launch(scene, film, params, direct):
    return rt.lib().rt_render_launch_direct(scene._p if scene is not None else None, film._p if film is not None else None,
                                            C.byref(params) if params is not None else None, C.byref(direct) if direct is not None else None)


def _params(width=W, height=H, spp=1):
    return _lib.RenderParams(width, height, spp, 6, 1984, 8, 0, 1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0)


def test_refusals_come_before_the_device_is_touched():
    scene = rt.builtin_scene(7, 0, W, H)
    # no film: refused as rt_render_launch refuses it, whatever `direct` holds -- its own checks come first
    for direct in (None, _lib.FilmDirectParams(2), _lib.FilmDirectParams(1)):
        assert abs(_launch(scene, None, _params(), direct)) == INVALID
        assert "rt_render_launch_direct" in rt.lib().rt_last_error().decode() and "null" in rt.lib().rt_last_error().decode()
    if not torch.cuda.is_available():
        with pytest.raises(rt.RtowError, match="no HIP device|HIP error"):   # a film cannot exist here: loudly
            rt.Film(W, H)


def test_refusals_that_need_a_film_name_their_field():
    if not torch.cuda.is_available():
        pytest.skip("a film cannot exist without a device (rt_film_create selects it): the refusals behind the NULL film run where one is")
    scene = rt.builtin_scene(7, 0, W, H)
    film = rt.Film(W, H)
    reserved = _lib.FilmDirectParams(1)
    reserved.reserved[6] = 1
    for direct, word in ((_lib.FilmDirectParams(2), "strategy"), (_lib.FilmDirectParams(-1), "strategy"), (reserved, "reserved"), (None, "direct")):
        assert abs(_launch(scene, film, _params(), direct)) == INVALID
        assert word in rt.lib().rt_last_error().decode()
    # the plain launch's refusals come first: a frame-size mismatch is named even where the strategy is wrong too
    assert abs(_launch(scene, film, _params(width=W + 1), _lib.FilmDirectParams(2))) == INVALID
    assert "geometry" in rt.lib().rt_last_error().decode()
    with pytest.raises(rt.RtowError, match="no direct launch"):   # nothing was launched by any of them
        film.direct_stats()
    with pytest.raises(rt.RtowError, match="nothing launched"):
        film.finish(scene)


def test_a_valid_launch_without_a_gpu_fails_loudly():
    if torch.cuda.is_available():
        return
    scene = rt.builtin_scene(7, 0, W, H)
    with pytest.raises(rt.RtowError, match="no HIP device|HIP error"):
        scene.render(W, H, 1, direct="mis")


def test_direct_is_none_or_mis():
    scene = rt.builtin_scene(7, 0, W, H)
    film = rt.Film.__new__(rt.Film)   # no device needed: the argument is refused before anything is called
    film.width, film.height, film.device, film.stripe_rows, film.rank, film.world_size, film._p = W, H, 0, 8, 0, 1, None
    for bad in ("nee", "MIS", True, 1):
        with pytest.raises(ValueError, match="direct"):
            film.render(scene, 1, direct=bad)
        with pytest.raises(ValueError, match="direct"):
            film.launch(scene, film.params(1), direct=bad)
        with pytest.raises(ValueError, match="direct"):
            scene.render(W, H, 1, direct=bad)
