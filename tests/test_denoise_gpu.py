"""The a-trous filter kernel (csrc/denoise.hip) against its numpy restatement (tests/test_denoise_host.py atrous_numpy), and the
film's filter path: equal to rt_denoise_frame on the film's downloads, never in place, refusing what it cannot do."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import api
from test_denoise_host import atrous_numpy

pytestmark = pytest.mark.gpu

SIGMAS = dict(sigma_color=0.9, sigma_albedo=0.8, sigma_normal=1.1, sigma_depth=0.7)
# (width, height): a single pixel; smaller than one tap row; smaller than level 1's footprint; odd and no tile multiple; larger
# than the step-16 footprint of 65 both ways, so that interior pixels see all 25 taps at every level
FRAMES = [(1, 1), (3, 2), (7, 5), (33, 17), (70, 66)]


def _inputs(width, height, seed):
    rng = np.random.default_rng(seed)
    normal = rng.standard_normal((height, width, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    return dict(color=1.5 * rng.random((height, width, 3)), albedo=rng.random((height, width, 3)), normal=normal,
                depth=1.0 + 4.0 * rng.random((height, width)))


def _tolerance(color):
    """|got - want| <= 1e-11 max(1, max |colour|): a tap's weight carries a few ulp from exp plus |e| eps exp(-e) <= eps / e from
    the rounding of its argument -- 25 taps x about 10 eps per level, over 5 levels."""
    return 1e-11 * max(1.0, float(np.abs(color[np.isfinite(color)]).max()))


@pytest.mark.parametrize("width,height", FRAMES)
def test_kernel_equals_the_numpy_restatement(width, height):
    """1 and 5 levels, all guides and each guide NULL in turn, seeded random inputs."""
    full = _inputs(width, height, 100 + width)
    worst = 0.0
    for iterations in (1, 5):
        for without in (None, "albedo", "normal", "depth"):
            g = {k: (None if k == without else v) for k, v in full.items()}
            got = api.denoise_frame(g["color"], g["albedo"], g["normal"], g["depth"], iterations=iterations, **SIGMAS)
            want = atrous_numpy(g["color"], g["albedo"], g["normal"], g["depth"], iterations, **SIGMAS)
            d = float(np.abs(got - want).max())
            worst = max(worst, d)
            assert np.isfinite(got).all()
            assert d <= _tolerance(full["color"]), (iterations, without, d)
    print(f"{width}x{height}: max |kernel - numpy| = {worst:.3g} (bound {_tolerance(full['color']):.3g})")


def test_infinite_sigmas_and_eight_levels():
    """A sigma of +inf is the factor 0: with all four the kernel is the B3 blur the restatement gives; 8 levels reach step 128, past
    this frame both ways."""
    g = _inputs(33, 17, 9)
    inf = float("inf")
    got = api.denoise_frame(g["color"], g["albedo"], g["normal"], g["depth"], iterations=8, sigma_color=inf, sigma_albedo=inf,
                            sigma_normal=inf, sigma_depth=inf)
    want = atrous_numpy(g["color"], iterations=8)
    assert np.abs(got - want).max() <= _tolerance(g["color"])
    mixed = api.denoise_frame(g["color"], g["albedo"], g["normal"], g["depth"], iterations=3, sigma_color=0.5, sigma_albedo=inf,
                              sigma_normal=0.7, sigma_depth=inf)
    assert np.abs(mixed - atrous_numpy(g["color"], None, g["normal"], None, 3, sigma_color=0.5, sigma_normal=0.7)).max() <= _tolerance(g["color"])


def test_nan_and_inf_colours_are_skipped_as_taps_and_pass_through_as_centres():
    g = _inputs(33, 17, 11)
    g["color"][5, 7, 1] = np.nan
    g["color"][11, 20, 0] = np.inf
    got = api.denoise_frame(g["color"], g["albedo"], g["normal"], g["depth"], iterations=5, **SIGMAS)
    want = atrous_numpy(g["color"], g["albedo"], g["normal"], g["depth"], 5, **SIGMAS)
    special = np.zeros((17, 33), dtype=bool)
    special[5, 7] = special[11, 20] = True
    assert np.array_equal(got[special].view(np.uint64), g["color"][special].view(np.uint64)), "the centre passes through unchanged"
    assert np.isfinite(got[~special]).all(), "a tap that is not finite has weight 0: it reaches no neighbour"
    d = float(np.abs(got[~special] - want[~special]).max())
    print(f"special values: max |kernel - numpy| = {d:.3g}")
    assert d <= _tolerance(g["color"])


W, H = 33, 17


@pytest.fixture(scope="module")
def scene():
    return rt.builtin_scene(7, 0, W, H)   # Cornell box + instances: flat walls, edges in albedo, normal and depth


def test_film_filter_equals_the_frame_filter_and_leaves_the_pixels_alone(scene):
    film = rt.Film(W, H)
    film.render(scene, 8, variant=0)
    film.render_features(scene, samples=0)
    raw = film.download()
    film.denoise(iterations=5, **SIGMAS)
    got = film.denoised()
    assert np.array_equal(film.download().view(np.uint64), raw.view(np.uint64)), "the filter never works in place"
    albedo, normal, depth = film.features()
    want = api.denoise_frame(raw, albedo, normal, depth, iterations=5, **SIGMAS)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "one kernel, the same planes: the same bits"
    assert np.abs(got - atrous_numpy(raw, albedo, normal, depth, 5, **SIGMAS)).max() <= _tolerance(raw)
    assert np.abs(got - raw).max() > 1e-3, "an 8-spp Cornell box is noisy: the filter moves it"
    film.denoise(iterations=1, **SIGMAS)   # (a single level writes the output buffer directly)
    assert np.array_equal(film.denoised().view(np.uint64), api.denoise_frame(raw, albedo, normal, depth, iterations=1, **SIGMAS).view(np.uint64))


def test_accumulated_frame_continues_after_a_denoise(scene):
    keep = rt.FLAG_KEEP_RNG_STATE | rt.FLAG_ACCUMULATE
    a, b = rt.Film(W, H), rt.Film(W, H)
    for film in (a, b):
        film.render(scene, 3, variant=0, flags=rt.FLAG_ACCUMULATE)
    a.render_features(scene, samples=2)
    a.denoise()
    for film in (a, b):
        film.render(scene, 3, variant=0, flags=keep)
    assert np.array_equal(a.download().view(np.uint64), b.download().view(np.uint64))
    whole, _ = scene.render(W, H, 6, variant=0)
    assert np.array_equal(a.download().view(np.uint64), whole.view(np.uint64))


def test_film_denoise_refusals(scene):
    """RT_ERR_STATE = 5 before a feature pass and while a launch is in flight, RT_ERR_UNSUPPORTED = 2 for a film that owns only
    part of the frame, RT_ERR_INVALID = 1 for parameters out of range."""
    film = rt.Film(W, H)
    with pytest.raises(api.RtowError, match="status 5"):
        film.denoise()
    with pytest.raises(api.RtowError, match="status 5"):
        film.features()
    assert film.device_features(0) is None
    film.render_features(scene)
    assert film.device_features(0) and film.device_features(1) and film.device_features(2) and film.device_features(3) is None
    with pytest.raises(api.RtowError, match="status 5"):
        film.denoised()
    with pytest.raises(api.RtowError, match="status 1"):
        film.denoise(iterations=0)
    with pytest.raises(api.RtowError, match="status 1"):
        film.denoise(sigma_depth=0.0)
    film.launch(scene, film.params(2))
    try:
        with pytest.raises(api.RtowError, match="status 5"):
            film.denoise()
        with pytest.raises(api.RtowError, match="status 5"):
            film.render_features(scene)
    finally:
        film.finish(scene)
    film.denoise()
    striped = rt.Film(W, H, stripe_rows=4, rank=1, world_size=2)
    striped.render_features(scene)
    with pytest.raises(api.RtowError, match="status 2"):
        striped.denoise()
    p = api.FeatureParams(W + 1, H, 0, 1984, 0, None)
    assert rt.lib().rt_film_render_features(scene._p, film._p, C.byref(p)) == 1
