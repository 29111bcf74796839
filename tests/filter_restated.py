"""The sphere-list scan's conservative filter (render.hip scan_ray / filter_s / filter_q / filter_behind and their packed fp32
form scan_ray32 / filter_pairs) restated in Python with the kernel's operation order, the reference's discriminant test
(R/Sphere.h:28-41) in plain double arithmetic, and the host's row of a sphere.  tests/test_filter_margin.py and
tests/test_filter_shared_axis.py hold the one against the other."""
import math
from fractions import Fraction

import numpy as np

F = np.float32


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                                    # infinities / NaNs propagate as in hardware
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # one rounding, like v_fma_f64


def dot(a, b):                                              # strict build: no contraction, left to right
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def scan_ray(o, d, reach):
    a = dot(d, d)
    oo = dot(o, o)
    w = math.sqrt(oo) + reach
    inv = 1.0 / math.sqrt(a)
    u = [inv * x for x in d]
    od = dot(o, u)
    p2 = [2.0 * (o[i] - od * u[i]) for i in range(3)]
    root_m = 2.0 ** -20 * w
    nthr = root_m * root_m - (oo - od * od)
    return dict(u=u, p2=p2, od=od, root_m=root_m, nthr=nthr)


def filter_pass(f, c, k):
    s = fma(c[2], f["u"][2], fma(c[1], f["u"][1], c[0] * f["u"][0]))
    q = fma(s, s, fma(f["p2"][2], c[2], fma(f["p2"][1], c[1], fma(f["p2"][0], c[0], f["nthr"]))))
    passed = q > k
    bu = f["od"] - s
    behind = passed and bu > f["root_m"] and fma(bu, bu, k - q) > 0.0
    return passed, behind


def reference(o, d, c, r2):
    oc = [o[i] - c[i] for i in range(3)]
    a = dot(d, d)
    b = dot(oc, d)
    cc = dot(oc, oc) - r2
    disc = b * b - a * cc
    return disc > 0.0, (b > 0.0 and cc > 0.0)


def host_row(c, r):
    r2 = r * r
    k = float(Fraction(c[0]) ** 2 + Fraction(c[1]) ** 2 + Fraction(c[2]) ** 2 - Fraction(r2))
    reach = (math.sqrt(dot(c, c)) + math.sqrt(r2)) * (1.0 + 2.0 ** -40)
    return r2, k, reach


# ---- the packed fp32 form: the same quantities, every operation rounded to fp32 ----
def fma32(a, b, c):
    """v_pk_fma_f32 / v_fma_f32: one rounding to fp32 (the exact product of two fp32 numbers fits a double; the sum is rounded
    to double and then to fp32 -- a double rounding that can differ from the fused one by half an fp32 ulp in 2^-29 of the cases:
    irrelevant to a margin that is 64 ulps wide)."""
    with np.errstate(all="ignore"):
        return F(np.float64(a) * np.float64(b) + np.float64(c))


def scan_ray32(o, d, reach):
    a = dot(d, d)
    oo = dot(o, o)
    w = math.sqrt(oo) + reach
    inv = 1.0 / math.sqrt(a)
    u = [inv * x for x in d]
    od = dot(o, u)
    p2 = [2.0 * (o[i] - od * u[i]) for i in range(3)]
    root_m = 2.0 ** -9 * w
    nthr = root_m * root_m - (oo - od * od)
    return dict(u=[F(x) for x in u], p2=[F(x) for x in p2], od=F(od), root_m=F(root_m), nthr=F(nthr))


def filter_pass32(f, c, k):
    cf = [F(x) for x in c]
    with np.errstate(all="ignore"):
        s = fma32(cf[2], f["u"][2], fma32(cf[1], f["u"][1], F(cf[0] * f["u"][0])))
        q = fma32(s, s, fma32(f["p2"][2], cf[2], fma32(f["p2"][1], cf[1], fma32(f["p2"][0], cf[0], f["nthr"]))))
        kf = F(k)
        passed = bool(q > kf)
        bu = F(f["od"] - s)
        behind = passed and bool(bu > f["root_m"]) and bool(fma32(bu, bu, F(kf - q)) > 0)
    return passed, behind
