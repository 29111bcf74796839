"""Adaptive sampling, host side (no GPU): the stopping rule the library exports (rt_adaptive_converged, compiled from the
source the kernel compiles: csrc/adaptive_rule.h) against a numpy restatement of include/rtow.h's description, parameter
validation, and the guard for the fixture the GPU tests (test_adaptive_gpu.py) stand on.

`predict_counts` is the rule applied to the CPU oracle's frames alone: a pixel's samples are one sequential random stream
and its sum is added in sample order, so "pixel (i, j) after n samples" is what the oracle's frame at spp = n holds, and the
radiance of sample k is k f_k^2 - (k - 1) f_{k-1}^2 (f = the stored sqrt(sum / k)); rebuilt that way the sums carry a relative
error of about 1e-13."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib

MIN, STEP, CAP, FLOOR = 16, 16, 128, 0.01


def rule_numpy(n, sr, sg, sb, q, min_samples, check_interval, tau, floor):
    """include/rtow.h, operation by operation (numpy never fuses a multiply with an add)."""
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        N = n.astype(np.float64)
        s = (sr + sg) + sb
        lhs = q * N - s * s
        fn = floor * N
        m = np.where(s > fn, s, fn)
        rhs = ((tau * tau) * (N - 1.0)) * (m * m)
        conv = lhs <= rhs   # False wherever a NaN is involved
    at_check = (n >= min_samples) & ((n - min_samples) % check_interval == 0)
    return conv & at_check


def rule_library(n, sr, sg, sb, q, min_samples, check_interval, tau, floor):
    p = _lib.AdaptiveParams(min_samples, check_interval, tau, floor)
    fn = rt.lib().rt_adaptive_converged
    ref = C.byref(p)
    return np.array([fn(ref, int(a), float(b), float(c), float(d), float(e)) for a, b, c, d, e in zip(n, sr, sg, sb, q)], dtype=np.int64)


def test_rule_equals_its_numpy_restatement_on_random_sums():
    rng = np.random.default_rng(1984)
    total = 0
    for min_samples, check_interval, tau, floor in ((16, 16, 0.05, 0.01), (2, 1, 0.25, 0.01), (32, 32, 1e-3, 0.5), (5, 7, 0.0, 1e-4),
                                                    (1000, 1, 0.05, 0.01)):
        k = 24000
        # mostly check points, some not, some below min_samples
        n = min_samples + check_interval * rng.integers(0, 12, k) + np.where(rng.random(k) < 0.15, rng.integers(-3, 4, k), 0)
        n = np.clip(n, 0, None)
        if min_samples >= 1000:   # a min_samples above every n
            n = rng.integers(0, min_samples, k)
        N = n.astype(np.float64)
        mean = rng.random((k, 3)) * np.array([0.7, 1.0, 1.3]) * np.where(rng.random(k) < 0.2, 1e-3, 1.0)[:, None]
        sr, sg, sb = (mean * N[:, None]).T
        s = (sr + sg) + sb
        m = np.maximum(s, floor * N)
        rhs = ((tau * tau) * (N - 1.0)) * (m * m)
        # q such that lhs lands around rhs: far below, far above, and within a few ulps of it
        f = np.where(rng.random(k) < 0.3, 1.0 + rng.integers(-4, 5, k) * 2.0 ** -52, np.exp(rng.normal(0.0, 1.0, k)))
        q = np.where(N > 0, (rhs * f + s * s) / np.maximum(N, 1.0), 0.0)
        want = rule_numpy(n, sr, sg, sb, q, min_samples, check_interval, tau, floor)
        got = rule_library(n, sr, sg, sb, q, min_samples, check_interval, tau, floor)
        assert np.array_equal(got, want.astype(np.int64)), (min_samples, check_interval, tau, floor, int(np.sum(got != want)))
        if min_samples < 1000:
            assert 0.05 < want.mean() < 0.95, "the random sums must fall on both sides of the rule"
        else:
            assert not got.any(), "min_samples above every n: never converged"
        total += k
    assert total >= 100000


def test_rule_on_the_edges():
    conv = lambda n, r, g, b, q, **kw: rt.adaptive_converged(n, r, g, b, q, **{**dict(min_samples=16, check_interval=16, noise_threshold=0.05,
                                                                                  luminance_floor=0.01), **kw})
    noisy = (32, 10.0, 11.0, 12.0, 100.0)          # s = 33, q N - s^2 = 2111 against 0.0025 * 31 * 1089 = 84.4
    quiet = (32, 10.0, 11.0, 12.0, 33.0 * 33.0 / 32.0 + 1.0)
    assert not conv(*noisy) and conv(*quiet)
    assert conv(16, *quiet[1:4], 33.0 * 33.0 / 16.0) and conv(48, *quiet[1:4], 33.0 * 33.0 / 48.0)  # at check points
    for n in (15, 17, 31, 33, 47):                  # off a check point, and below min_samples
        assert not conv(n, *quiet[1:])
    assert not conv(8, 1.0, 1.0, 1.0, 0.0)
    # q N = s^2 exactly (all samples equal, exactly representable): lhs = 0 <= rhs, also at tau = 0
    assert conv(16, 8.0, 4.0, 4.0, 16.0) and conv(16, 8.0, 4.0, 4.0, 16.0, noise_threshold=0.0)
    assert not conv(16, 8.0, 4.0, 4.0, 16.0 + 2.0 ** -40, noise_threshold=0.0)
    # a black pixel converges through the luminance floor
    assert conv(16, 0.0, 0.0, 0.0, 0.0) and conv(32, 0.0, 0.0, 0.0, 0.0)
    # a NaN anywhere: not converged
    nan = float("nan")
    assert not conv(16, nan, 1.0, 1.0, 1.0) and not conv(16, 1.0, 1.0, 1.0, nan) and not conv(16, 1.0, nan, 1.0, nan)
    # min_samples above any n: never (what the overhead measurement of profiles/adaptive_measure.py uses)
    assert not conv(128, 0.0, 0.0, 0.0, 0.0, min_samples=1 << 30)
    # the numpy restatement says the same of every case above
    for args in (noisy, quiet, (16, 0.0, 0.0, 0.0, 0.0), (16, nan, 1.0, 1.0, 1.0), (16, 8.0, 4.0, 4.0, 16.0)):
        n, r, g, b, q = args
        assert bool(rule_numpy(np.array([n]), np.array([r]), np.array([g]), np.array([b]), np.array([q]), 16, 16, 0.05, 0.01)[0]) == conv(*args)


@pytest.mark.parametrize("bad", [dict(min_samples=1), dict(min_samples=0), dict(min_samples=-5), dict(check_interval=0), dict(check_interval=-1),
                                 dict(noise_threshold=-1e-9), dict(noise_threshold=float("nan")), dict(luminance_floor=0.0),
                                 dict(luminance_floor=-0.01), dict(luminance_floor=float("nan"))])
def test_parameters_out_of_range_are_invalid(bad):
    """rt_adaptive_converged validates without a device, with the check rt_film_set_adaptive applies (test_adaptive_gpu.py asks that one too)."""
    good = dict(min_samples=2, check_interval=1, noise_threshold=0.0, luminance_floor=1e-9)
    assert rt.adaptive_converged(2, 1.0, 1.0, 1.0, 4.5, **good) in (True, False)
    p = _lib.AdaptiveParams(**{**good, **bad})
    assert rt.lib().rt_adaptive_converged(C.byref(p), 16, 1.0, 1.0, 1.0, 1.0) == -1   # -RT_ERR_INVALID
    with pytest.raises(rt.RtowError, match="status 1"):
        rt.adaptive_converged(16, 1.0, 1.0, 1.0, 1.0, **{**good, **bad})
    assert rt.lib().rt_adaptive_converged(None, 16, 1.0, 1.0, 1.0, 1.0) == -1


# ---- the rule on the oracle's frames ----
def oracle_frames(oracle, scene_id, world_kind, w, h, cap=CAP, earth=None):
    """The oracle's frames at 1 .. cap samples per pixel, (cap + 1, h, w, 3) with a row of zeros in front."""
    return np.stack([np.zeros((h, w, 3))] + [oracle.render(scene_id, world_kind, w, h, k, earth=earth) for k in range(1, cap + 1)])


def predict_counts(frames, tau, min_samples=MIN, check_interval=STEP, floor=FLOOR):
    """(counts, closest |lhs - rhs| / rhs over the checks each pixel reached) for a cap of len(frames) - 1."""
    cap = frames.shape[0] - 1
    k = np.arange(cap + 1, dtype=np.float64)[:, None, None, None]
    sums = frames * frames * k
    samp = sums[1:] - sums[:-1]
    y = (samp[..., 0] + samp[..., 1]) + samp[..., 2]
    q = np.cumsum(y * y, axis=0)
    s = (sums[1:, ..., 0] + sums[1:, ..., 1]) + sums[1:, ..., 2]
    count = np.full(frames.shape[1:3], cap, dtype=np.int64)
    done = np.zeros(frames.shape[1:3], dtype=bool)
    gap = np.full(frames.shape[1:3], np.inf)
    for n in range(min_samples, cap, check_interval):   # (the check at the cap itself cannot change a count)
        sn, qn, N = s[n - 1], q[n - 1], float(n)
        lhs = qn * N - sn * sn
        m = np.maximum(sn, floor * N)
        rhs = ((tau * tau) * (N - 1.0)) * (m * m)
        with np.errstate(all="ignore"):
            gap = np.where(done, gap, np.minimum(gap, np.abs(lhs - rhs) / rhs))
        newly = (lhs <= rhs) & ~done
        count[newly] = n
        done |= newly
    return count, gap


def test_fixture_guard_three_spheres(oracle):
    """The inputs of the GPU tests are not vacuous: scene 10 as a list world at 48 x 32, tau = 0.05 has pixels stopping at at
    least four different counts, the first check and the cap among them, and none within 1e-6 (relative) of the threshold."""
    frames = oracle_frames(oracle, 10, 1, 48, 32)
    count, gap = predict_counts(frames, 0.05)
    values, pixels = np.unique(count, return_counts=True)
    print(dict(zip(values.tolist(), pixels.tolist())), "closest", gap.min())
    assert len(values) >= 4 and MIN in values and CAP in values
    assert set(values.tolist()) <= set(range(MIN, CAP + 1, STEP))
    assert gap.min() > 1e-6
    # the issue's table for this row
    assert dict(zip(values.tolist(), pixels.tolist())) == {16: 673, 32: 134, 48: 91, 64: 81, 80: 71, 96: 58, 112: 53, 128: 375}
