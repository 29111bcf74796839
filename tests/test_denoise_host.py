"""The edge-avoiding a-trous filter (include/rtow.h rt_denoise_params) restated in numpy, and what of the new calls can be checked
without a device.  ``atrous_numpy`` is the reference the GPU tests compare the kernel with (tests/test_denoise_gpu.py)."""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import api

INF = float("inf")
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def _dist_sq(a, b):
    d = a - b
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]   # the plain three-term sum


def atrous_numpy(color, albedo=None, normal=None, depth=None, iterations=5, sigma_color=INF, sigma_albedo=INF, sigma_normal=INF,
                 sigma_depth=INF):
    """The filter as include/rtow.h states it, tap by tap in the stated order (dy outer, dx inner, ascending), every pixel at once.
    A guide that is None switches its term off.  A tap whose colour is not finite has weight 0; a centre whose colour is not
    finite passes through."""
    c = np.array(color, dtype=np.float64)
    height, width = c.shape[:2]
    a = None if albedo is None else np.asarray(albedo, dtype=np.float64)
    n = None if normal is None else np.asarray(normal, dtype=np.float64)
    z = None if depth is None else np.asarray(depth, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(iterations):
            step = 1 << k
            sck = sigma_color * 2.0 ** -k
            num = np.zeros((height, width, 3))
            den = np.zeros((height, width))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * step, dx * step
                    y0, y1, x0, x1 = max(0, -oy), min(height, height - oy), max(0, -ox), min(width, width - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue   # every such tap lies outside the frame
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    cq = c[q]
                    e = _dist_sq(c[p], cq) / (sck * sck)
                    if a is not None:
                        e = e + _dist_sq(a[p], a[q]) / (sigma_albedo * sigma_albedo)
                    if n is not None:
                        e = e + _dist_sq(n[p], n[q]) / (sigma_normal * sigma_normal)
                    if z is not None:
                        r = (z[p] - z[q]) / np.maximum(np.maximum(z[p], z[q]), 1e-30)
                        e = e + (r * r) / (sigma_depth * sigma_depth)
                    ok = np.isfinite(cq).all(axis=-1)
                    w = np.where(ok, (H5[dx + 2] * H5[dy + 2]) * np.exp(-e), 0.0)
                    num[p] += w[..., None] * np.where(ok[..., None], cq, 0.0)
                    den[p] += w
            out = num / den[..., None]
            through = ~np.isfinite(c).all(axis=-1)
            out[through] = c[through]
            c = out
    return c


def test_constant_image_is_a_fixed_point():
    """Every weight multiplies the same colour: out = (sum w c) / (sum w) = c, with random guides shaping the weights, a frame
    smaller than the last level's footprint (border renormalisation at every level) and five levels.
    To 1 ulp where the arithmetic allows it: a channel that is a power of two makes every product w c a scaling, exact, so
    sum (w c) is c (sum w) bit for bit and the quotient is c -- any error there is the filter's (a tap counted in one sum and not
    in the other, a weight normalised twice), not rounding's.  For a channel with a full mantissa the 25 products and 24
    additions of a level round (at most 50 eps relative for terms of one sign, plus the quotient's half), five levels on top of each
    other: 5 x 51 eps is the bound there, and the measured worst is printed (11 ulp for these inputs)."""
    rng = np.random.default_rng(5)
    guides = (rng.random((13, 17, 3)), rng.standard_normal((13, 17, 3)), 1.0 + rng.random((13, 17)))
    color = np.empty((13, 17, 3))
    color[:] = (0.25, 2.0, 0.5)
    out = atrous_numpy(color, *guides, 5, 0.6, 0.5, 0.8, 0.4)
    ulps = np.abs(out - color) / np.spacing(color)
    print("constant image, power-of-two channels: worst", ulps.max(), "ulp")
    assert ulps.max() <= 1.0
    color[:] = (0.3, 0.625, 0.9)
    out = atrous_numpy(color, *guides, 5, 0.6, 0.5, 0.8, 0.4)
    print("constant image, full mantissas: worst", (np.abs(out - color) / np.spacing(color)).max(), "ulp")
    assert (np.abs(out - color) / color).max() <= 5 * 51 * np.finfo(np.float64).eps


def _b3_blur(color):
    """Separable B3 blur with border renormalisation: rows, then columns, each normalised by the kernel weight inside the frame."""
    def along(img, axis):
        img = np.moveaxis(img, axis, 0)
        num, den = np.zeros_like(img), np.zeros(img.shape[0])
        for d in range(-2, 3):
            lo, hi = max(0, -d), min(img.shape[0], img.shape[0] - d)
            num[lo:hi] += H5[d + 2] * img[lo + d:hi + d]
            den[lo:hi] += H5[d + 2]
        return np.moveaxis(num / den.reshape(-1, *([1] * (img.ndim - 1))), 0, axis)
    return along(along(color, 1), 0)


def test_all_sigmas_infinite_is_the_b3_blur():
    """Every exponent is an exact 0, every weight h[dx] h[dy]: one level is the separable B3 blur, renormalised at the border.  Two
    orders of summing 25 terms of like sign: 25 roundings each, 60 eps relative is generous for both."""
    rng = np.random.default_rng(6)
    color = rng.random((9, 14, 3))
    guides = (rng.random((9, 14, 3)), rng.standard_normal((9, 14, 3)), 1.0 + rng.random((9, 14)))
    out = atrous_numpy(color, *guides, iterations=1)
    want = _b3_blur(color)
    assert np.abs(out - want).max() <= 60 * np.finfo(np.float64).eps
    assert np.array_equal(out, atrous_numpy(color, iterations=1))   # the guides' terms were exact zeros


def test_no_colour_crosses_an_albedo_edge():
    """Two albedo regions, sigma_albedo tiny: exp(-3 / 1e-4) underflows to 0, so no output left of the edge depends on any colour
    right of it -- changing the right half's colours changes the left half's outputs by exactly 0, and the other way round."""
    rng = np.random.default_rng(7)
    height, width, edge = 11, 20, 9
    albedo = np.zeros((height, width, 3))
    albedo[:, edge:] = 1.0
    color = rng.random((height, width, 3))
    other = color.copy()
    other[:, edge:] = 5.0 + rng.random((height, width - edge, 3))
    kw = dict(albedo=albedo, iterations=4, sigma_color=INF, sigma_albedo=1e-2)
    a, b = atrous_numpy(color, **kw), atrous_numpy(other, **kw)
    leak = np.abs(a[:, :edge] - b[:, :edge]).max()
    assert leak == 0.0
    assert (b[:, edge:] >= 5.0).all() and (a[:, :edge] <= 1.0).all()
    smooth = atrous_numpy(color, iterations=4)   # without the guide the halves do mix
    assert np.abs(smooth[:, :edge] - atrous_numpy(other, iterations=4)[:, :edge]).max() > 0.1


@pytest.mark.parametrize("bad", [dict(iterations=0), dict(iterations=9), dict(sigma_color=0.0), dict(sigma_albedo=-1.0),
                                 dict(sigma_normal=float("nan")), dict(sigma_depth=0.0)])
def test_denoise_frame_refuses_bad_parameters_before_it_needs_a_device(bad):
    """RT_ERR_INVALID = 1 for iterations outside 1..8 and for a sigma that is not > 0; the check comes before the device is
    touched, so it is the same answer with and without one.  (The refusals of rt_film_denoise need a film, and a film a device:
    tests/test_denoise_gpu.py.)"""
    with pytest.raises(api.RtowError, match="status 1"):
        api.denoise_frame(np.zeros((4, 4, 3)), **bad)


def test_denoise_frame_refuses_null_arrays_and_bad_sizes():
    p = api.DenoiseParams(1, 1.0, 1.0, 1.0, 1.0)
    out = np.zeros(3)
    import ctypes as C
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    assert rt.lib().rt_denoise_frame(0, None, None, None, None, 1, 1, C.byref(p), ptr) == 1
    assert rt.lib().rt_denoise_frame(0, ptr, None, None, None, 0, 1, C.byref(p), ptr) == 1
    assert rt.lib().rt_denoise_frame(0, ptr, None, None, None, 1, 1, None, ptr) == 1
    assert rt.lib().rt_film_denoise(None, C.byref(p)) == 1
    assert rt.lib().rt_film_render_features(None, None, None) == 1
    assert rt.lib().rt_film_device_features(None, 0) is None
