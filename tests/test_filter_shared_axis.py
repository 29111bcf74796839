"""The packed fp32 filter's shared-coordinate form (render.hip filter_pairs<true>, set up per run segment in scan_filtered32),
restated operation by operation as tests/filter_restated.py restates the general form: every product-sum exact, one rounding
to fp32 per operation.

In a run of rows that share the centre coordinate c on one axis, the two multiply-adds that involve only c are formed once per
ray -- s0 = c u, l0 = fma(p, c, nt) -- and each row then costs two multiply-adds for s and three for q:

    s = fma(cj, uj, fma(ci, ui, s0))        q = fma(s, s, fma(pj, cj, fma(pi, ci, l0)))        (i < j the two other axes)

The property is the general form's: whenever the reference's `disc > 0` holds and the sphere is not outside-and-behind, the
filter passes it and does not call it behind.  Margins, M and root_m are the general form's, untouched.
"""
import math

import numpy as np
import pytest

from filter_restated import F, dot, fma32, host_row, reference, scan_ray32


def run_setup(f, axis, shared):
    """Once per ray and run segment: the shared coordinate's share of both chains."""
    with np.errstate(all="ignore"):
        return F(shared * f["u"][axis]), fma32(f["p2"][axis], shared, f["nthr"])


def filter_pass_run(f, axis, s0, l0, c, k):
    """One row of the run: c is the sphere's centre; the row holds fl32 of its two other coordinates and never the shared one."""
    i, j = [a for a in range(3) if a != axis]
    ci, cj = F(c[i]), F(c[j])
    with np.errstate(all="ignore"):
        s = fma32(cj, f["u"][j], fma32(ci, f["u"][i], s0))
        q = fma32(s, s, fma32(f["p2"][j], cj, fma32(f["p2"][i], ci, l0)))
        kf = F(k)
        passed = bool(q > kf)
        bu = F(f["od"] - s)
        behind = passed and bool(bu > f["root_m"]) and bool(fma32(bu, bu, F(kf - q)) > 0)
    return passed, behind


OFFSETS = [((0.0, 0.0, 0.0), 1.0, 11.0), ((13.0, 2.0, 3.0), 1.0, 11.0), ((300.0, -200.0, 500.0), 1.0, 11.0),
           ((0.0, 0.0, 0.0), 0.01, 3.0), ((0.0, 0.0, 0.0), 50.0, 400.0)]   # test_filter_margin's, for the fp32 form
EPS = [0.0, 1e-16, -1e-16, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-3, -1e-3, 0.3, -0.3]
TRIALS = 400


@pytest.mark.parametrize("shared", [0.0, 0.2, -7.3, 1e3])
@pytest.mark.parametrize("offset,scale,spread", OFFSETS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_run_form_never_rejects_what_the_reference_accepts(axis, offset, scale, spread, shared):
    """Spheres whose centre has fl32(`shared`) on `axis` -- the bit-same value the segment record carries -- and anything on the
    other two; rays that pass them at r (1 + eps), eps from far outside to far inside through zero, from origins near and far."""
    rng = np.random.default_rng(1000 * axis + 17)
    cs = float(F(shared))          # the spheres of a run have exactly this coordinate in fp32; so has this one in fp64
    accepted = grazing = 0
    for trial in range(TRIALS):
        c = [offset[i] + float(rng.uniform(-spread, spread)) for i in range(3)]
        c[axis] = cs
        r = scale * float(rng.choice([0.2, 1.0, 0.5]))
        r2, k, reach_c = host_row(c, r)
        reach32 = max(reach_c, (math.sqrt(dot(offset, offset)) + 1.8 * spread + scale) * (1.0 + 2.0 ** -20))   # the bulk's reach
        far = float(rng.choice([1.0, 1.0, 10.0, 1000.0]))
        o = [offset[i] + far * float(rng.uniform(-15, 15)) for i in range(3)]
        tdir = rng.normal(size=3)
        to_c = np.array(c) - np.array(o)
        perp = np.cross(to_c, tdir)
        perp /= np.linalg.norm(perp)
        eps = float(rng.choice(EPS))
        target = np.array(c) + perp * r * (1.0 + eps)
        d = (target - np.array(o)) * float(rng.uniform(0.2, 3.0)) * float(rng.choice([1.0, -1.0]))
        d = [float(x) for x in d]
        f = scan_ray32(o, d, reach32)
        s0, l0 = run_setup(f, axis, F(cs))
        ok, behind = filter_pass_run(f, axis, s0, l0, c, k)
        acc, ref_behind = reference(o, d, c, r2)
        if acc and not ref_behind:
            accepted += 1
            assert ok and not behind, (axis, o, d, c, r, eps)
        if behind:
            assert (not acc) or ref_behind, "the run form calls a sphere behind that the reference would test"
        grazing += abs(eps) <= 1e-6
    # not vacuous: 11 of the 17 eps are grazing (260 of 400 trials); 6 of 17 lie inside by more than fp64 can blur, and half the
    # rays point towards the sphere (70 of 400).  Half of either expectation is far below what chance takes away.
    assert accepted > 35 and grazing > 130


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_shared_coordinate_rounded_from_fp64_keeps_the_property(axis):
    """C2's plane: the spheres' y is the double 0.2, the rows' and the segment's is fl32(0.2), as for every other coordinate of
    the general form (centres are rounded to fp32 there too, within the same margin)."""
    rng = np.random.default_rng(5 + axis)
    accepted = 0
    for trial in range(1500):
        c = [float(rng.uniform(-11, 11)) for _ in range(3)]
        c[axis] = 0.2
        r2, k, _ = host_row(c, 0.2)
        o = [13.0, 2.0, 3.0] if trial % 2 else [float(rng.uniform(-11, 11)), float(rng.uniform(0, 2)), float(rng.uniform(-11, 11))]
        perp = np.cross(np.array(c) - np.array(o), rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        eps = float(rng.choice(EPS))
        d = [float(x) for x in (np.array(c) + perp * 0.2 * (1.0 + eps) - np.array(o)) * float(rng.choice([1.0, -1.0]))]
        f = scan_ray32(o, d, 16.5)
        s0, l0 = run_setup(f, axis, F(0.2))
        ok, behind = filter_pass_run(f, axis, s0, l0, c, k)
        acc, ref_behind = reference(o, d, c, r2)
        if acc and not ref_behind:
            accepted += 1
            assert ok and not behind, (axis, o, d, c, eps)
    assert accepted > 300


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_degenerate_rays_and_undecided_rows(axis):
    """scan_ray32's `sane` false: u = p = 0, nthr = +inf, root_m = +inf: every decided row passes and none is behind.  A row with
    k = -inf (zeros for a centre) passes for every ray and is never behind; a padding row (k = +inf) never passes."""
    inf = F(np.inf)
    f = dict(u=[F(0)] * 3, p2=[F(0)] * 3, od=F(0), root_m=inf, nthr=inf)
    s0, l0 = run_setup(f, axis, F(-7.3))
    assert filter_pass_run(f, axis, s0, l0, [1.0, 2.0, 3.0], 13.0) == (True, False)
    assert filter_pass_run(f, axis, s0, l0, [0.0, 0.0, 0.0], np.inf) == (False, False)
    g = scan_ray32([13.0, 2.0, 3.0], [-1.0, -0.1, -0.3], 16.5)
    s0, l0 = run_setup(g, axis, F(1e3))
    assert filter_pass_run(g, axis, s0, l0, [0.0, 0.0, 0.0], -np.inf) == (True, False)
    assert filter_pass_run(g, axis, s0, l0, [0.0, 0.0, 0.0], np.inf) == (False, False)
