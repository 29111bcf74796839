"""The environment restated in numpy, operation by operation as include/rtow.h states it (rt_scene_set_environment,
rt_scene_dump_environment_cdf, rt_scene_sample_environment, rt_scene_environment_pdf): what the strict build must return.  numpy's
elementwise operations are single IEEE-754 double operations and nothing is fused, like the strict build; sums "in order" go
through np.cumsum, which adds left to right.  acos, atan2, sin and cos are each library's own: the tests that compare through them
say how.  Shared by tests/test_environment_host.py and tests/test_environment_gpu.py."""
import math

import numpy as np

from light_restated import PI, Streams, usable

IDENTITY = np.eye(3)


def rotation(axis, degrees):
    """A rotation about ``axis`` (not axis-aligned unless the axis is), orthonormal to a few ulp (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt(a @ a)
    t = math.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def coords(d, R=IDENTITY):
    """n, e = R n and (u, v) = GetSphereUV(e) of the directions d (count, 3)."""
    d = np.asarray(d, dtype=np.float64)
    n = (1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None] * d
    e = np.stack([(R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2] for r in range(3)], axis=-1)
    with np.errstate(invalid="ignore"):
        theta = np.arccos(-e[:, 1])
        phi = np.arctan2(-e[:, 2], e[:, 0]) + PI
    return e, phi / (2.0 * PI), theta / PI


def texel(W, H, u, v):
    """ImageTexture::Value's index rule: (i, j), j counted from the top row."""
    u = np.where(u < 0.0, 0.0, np.where(u > 1.0, 1.0, u))
    v = np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))
    v = 1.0 - v
    i = np.clip((u * W).astype(np.int64), 0, W - 1)
    j = np.clip((v * H).astype(np.int64), 0, H - 1)
    return i, j


def texel_is_stable(W, H, u, v, ulps=4):
    """Does (u, v) moved by +-``ulps`` units in the last place still name the same texel?  (acos and atan2 are each library's own.)"""
    i, j = texel(W, H, u, v)
    ok = np.ones(len(u), dtype=bool)
    for su in (-1, 1):
        for sv in (-1, 1):
            uu, vv = u.copy(), v.copy()
            for _ in range(ulps):
                uu = np.nextafter(uu, su * np.inf)
                vv = np.nextafter(vv, sv * np.inf)
            i2, j2 = texel(W, H, uu, vv)
            ok &= (i2 == i) & (j2 == j)
    return ok


def image_values(image):
    """The texel values as doubles: a float image widened, an 8-bit image as (1.0 / 255.0) * byte."""
    image = np.asarray(image)
    return (1.0 / 255.0) * image.astype(np.float64) if image.dtype == np.uint8 else image.astype(np.float64)


def image_value(image, intensity, u, v):
    """intensity * texel, for a float32 or uint8 (H, W, 3) image, top row first."""
    values = image_values(image)
    H, W = values.shape[:2]
    i, j = texel(W, H, u, v)
    return np.asarray(intensity, dtype=np.float64)[None, :] * values[j, i]


def checker_value(inv_scale, even, odd, intensity, e):
    """intensity * a checker of two solid colours at the point e (R/Texture.h:70-81)."""
    n = np.floor(inv_scale * e[:, 0]).astype(np.int64) + np.floor(inv_scale * e[:, 1]).astype(np.int64) + np.floor(inv_scale * e[:, 2]).astype(np.int64)
    c = np.where((n % 2 == 0)[:, None], np.asarray(even, dtype=np.float64)[None, :], np.asarray(odd, dtype=np.float64)[None, :])
    return np.asarray(intensity, dtype=np.float64)[None, :] * c


def centre_directions(W, H, R=IDENTITY, length=1.0):
    """One direction through the centre of every texel, row by row from the top: (H * W, 3), world space."""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u = ((i + 0.5) / W).reshape(-1)
    v = (1.0 - (j + 0.5) / H).reshape(-1)
    theta, phi = PI * v, 2.0 * PI * u - PI
    e = np.stack([np.sin(theta) * np.cos(phi), -np.cos(theta), -(np.sin(theta) * np.sin(phi))], axis=-1)
    return length * (e @ R)  # R^T e per row


def build_cdf(image, intensity):
    """(marginal (H,), conditional (H, W)) of rt_scene_dump_environment_cdf, or None where there is no distribution."""
    values = image_values(image)
    H, W = values.shape[:2]
    k = np.asarray(intensity, dtype=np.float64)
    x = k[None, None, :] * values
    brightest = np.where(x[..., 1] > x[..., 0], x[..., 1], x[..., 0])
    brightest = np.where(x[..., 2] > brightest, x[..., 2], brightest)
    sn = np.array([math.sin(PI * (j + 0.5) / H) for j in range(H)])   # the host's libm, as the library's
    w = brightest * sn[:, None]
    part = np.cumsum(w, axis=1)
    row_sum = part[:, -1]
    run = np.cumsum(row_sum)
    total = run[-1]
    if not (np.isfinite(total) and total > 0.0):
        return None
    marginal = run / total
    marginal[-1] = 1.0
    conditional = np.ones((H, W))
    live = row_sum > 0.0
    conditional[live] = part[live] / row_sum[live][:, None]
    conditional[:, -1] = 1.0
    return marginal, conditional


def first_at_least(table, x):
    """Per row k: the first index with table[k, idx] >= x[k] (table rows end at 1.0 >= x)."""
    return np.argmax(table >= x[:, None], axis=1)


def density(cdf, W, H, e, u, v):
    """(pdf, texel) of the direction whose environment coordinates are e, (u, v); cdf None: the uniform sphere."""
    if cdf is None:
        return np.full(len(u), 1.0 / (4.0 * PI)), np.full(len(u), -1, dtype=np.int64)
    marginal, conditional = cdf
    i, j = texel(W, H, u, v)
    pj = marginal[j] - np.where(j > 0, marginal[np.maximum(j - 1, 0)], 0.0)
    pi = conditional[j, i] - np.where(i > 0, conditional[j, np.maximum(i - 1, 0)], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pdf = ((pj * pi) * (float(W) * float(H))) / (((2.0 * PI) * PI) * np.sqrt(1.0 - e[:, 1] * e[:, 1]))
    return pdf, j * W + i


def sample(cdf, W, H, states, R=IDENTITY):
    """rt_scene_sample_environment up to the direction: dict with the four draws' results -- "texel" (j * W + i, -1 without a
    distribution), "direction" (R^T e, through numpy's sin and cos), "pdf" and "valid" of that direction, "rng_state"."""
    rng = Streams(states)
    a, b, c, d = rng.uniform(), rng.uniform(), rng.uniform(), rng.uniform()
    n = len(a)
    if cdf is not None:
        marginal, conditional = cdf
        j = first_at_least(np.broadcast_to(marginal, (n, H)), a)
        i = first_at_least(conditional[j], b)
        tex = j * W + i
        u = (i + c) / float(W)
        v = 1.0 - (j + d) / float(H)
        theta, phi = PI * v, (2.0 * PI) * u - PI
        st = np.sin(theta)
        e = np.stack([st * np.cos(phi), -np.cos(theta), -(st * np.sin(phi))], axis=-1)
    else:
        tex = np.full(n, -1, dtype=np.int64)
        y = 1.0 - 2.0 * c
        st, phi = np.sqrt(1.0 - y * y), (2.0 * PI) * d - PI
        e = np.stack([st * np.cos(phi), y, -(st * np.sin(phi))], axis=-1)
    direction = np.stack([(R[0, r] * e[:, 0] + R[1, r] * e[:, 1]) + R[2, r] * e[:, 2] for r in range(3)], axis=-1)
    el, u2, v2 = coords(direction, R)
    pdf, seen = density(cdf, W, H, el, u2, v2)
    valid = usable(pdf)
    return {"texel": tex, "direction": np.where(valid[:, None], direction, 0.0), "pdf": np.where(valid, pdf, 0.0), "valid": valid,
            "seen": seen, "rng_state": rng.s}


def integral(image, intensity):
    """The map's exact integral over the sphere per channel: sum L_ij * (2 pi / W) * (cos(theta_j0) - cos(theta_j1))."""
    L = np.asarray(intensity, dtype=np.float64)[None, None, :] * image_values(image)
    H, W = L.shape[:2]
    j = np.arange(H)
    band = np.cos(PI * j / H) - np.cos(PI * (j + 1) / H)
    return (L * ((2.0 * PI / W) * band)[:, None, None]).sum(axis=(0, 1))
