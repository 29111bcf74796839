"""Sphere lists placed against the window rule of the sphere-list scan (csrc/scan_window_rule.h; scene_builder.cpp
build_scan_windows), with what each must give, the reference's sphere test restated in numpy, and the check both
tests/test_scan_windows_host.py and tests/test_list_scan_windows_gpu.py make on a list's tables.  Not a test module."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt
import scan_segment_lists as S

TRIP = S.TRIP
W, H = S.W, S.H
MAX_MEAN_SPAN = 0.25  # scan_window_rule.h kScanWindowMaxMeanSpan


def row(rnd, n, axis, shared, along, lo, hi, order="up", radius=(0.15, 0.25)):
    """n small spheres whose centres share `shared` on `axis` and are spread evenly over [lo, hi] on `along` (a little jitter),
    random on the third axis: in ascending, descending or random list order."""
    third = 3 - axis - along
    at = np.linspace(lo, hi, n) + rnd.uniform(-0.05, 0.05, n)
    if order == "down":
        at = at[::-1]
    elif order == "random":
        at = rnd.permutation(at)
    out = []
    for k in range(n):
        c = [0.0, 0.0, 0.0]
        c[axis] = shared
        c[along] = float(at[k])
        c[third] = float(rnd.uniform(-9.0, -3.0) if third == 2 else rnd.uniform(-3.0, 3.0) if third == 0 else rnd.uniform(-0.4, 1.2))
        out.append((tuple(c), float(rnd.uniform(*radius))))
    return out


def _cases():
    """name -> (spheres in list order, per segment: None for a segment that must have no table, else the window axis)."""
    rnd = np.random.default_rng(20291)
    cases = {}
    cases["ascending_on_y"] = (row(rnd, 64, 1, 0.3, 0, -6.0, 6.0), [0])
    cases["descending_on_y"] = (row(rnd, 64, 1, 0.3, 0, -6.0, 6.0, order="down"), [0])
    cases["random_order"] = (row(rnd, 64, 1, 0.3, 0, -6.0, 6.0, order="random"), [None])
    cases["mixed_radii"] = (row(rnd, 64, 1, 0.3, 0, -6.0, 6.0, radius=(0.05, 0.6)), [0])
    giant = row(rnd, 64, 1, 0.3, 0, -6.0, 6.0)
    giant[29] = S.GROUND
    cases["undecided_giant_inside"] = (giant, [0])
    cases["run_on_x_along_z"] = (row(rnd, 64, 0, 0.5, 2, -12.0, -3.0), [2])
    cases["run_on_z_along_y"] = (row(rnd, 64, 2, -6.0, 1, -3.0, 4.0), [1])
    cases["more_than_64_trips"] = (row(rnd, 66 * TRIP + 3, 1, 0.3, 0, -30.0, 30.0), [0])
    cases["two_runs_general_between"] = (row(rnd, 48, 1, 0.3, 0, -6.0, 6.0) + S.field(rnd, 16) + row(rnd, 48, 1, 0.9, 2, -12.0, -3.0), [0, None, 2])
    # 61 rows: the run's last trip ends in three rows of padding
    cases["padding_at_the_end"] = (row(rnd, 61, 1, 0.3, 0, -6.0, 6.0), [0])
    return cases


CASES = _cases()


def quarter(step):
    """Four trips on y whose spans on x are each 1 wide (two rows at either end, radius 0.25, the rest between) and `step` apart:
    mean span / extent = 1 / (3 step + 1), a quarter at step = 1.  On z every trip covers the whole range."""
    out = []
    for t in range(4):
        xs = [t * step, t * step + 0.5] + [t * step + 0.0625 * k for k in range(1, 7)]
        zs = [-9.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0, -3.5]
        out += [((x, 0.3, z), 0.25) for x, z in zip(xs, zs)]
    return out


def scene11():
    """Scene 11 as a list (config C2) and its spheres as the world's leaves give them back: ((centre), radius) in list order."""
    s = rt.builtin_scene(11, 1, 1200, 800)
    kinds, boxes = s.dump_leaves()
    assert all(k == 0 for k in kinds)
    return s, [((0.5 * (b[0] + b[1]), 0.5 * (b[2] + b[3]), 0.5 * (b[4] + b[5])), 0.5 * (b[1] - b[0])) for b in boxes]


def reference_accepts(o, d, spheres, tmin=0.001):
    """The reference's Sphere::Hit (R/Sphere.h:29-58) over (tmin, inf) in plain fp64, one operation at a time, for every ray against
    every sphere: a bool array (rays, spheres)."""
    c = np.array([s[0] for s in spheres], dtype=np.float64)
    r = np.array([s[1] for s in spheres], dtype=np.float64)
    with np.errstate(all="ignore"):
        oc = o[:, None, :] - c[None, :, :]
        dd = d[:, None, :]
        a = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
        b = (oc[..., 0] * dd[..., 0] + oc[..., 1] * dd[..., 1]) + oc[..., 2] * dd[..., 2]
        cc = ((oc[..., 0] * oc[..., 0] + oc[..., 1] * oc[..., 1]) + oc[..., 2] * oc[..., 2]) - (r * r)[None, :]
        disc = b * b - a * cc
        root = np.sqrt(np.where(disc > 0.0, disc, 0.0))
        t1, t2 = (-b - root) / a, (-b + root) / a
        return (disc > 0.0) & (((t1 > tmin) & (t1 < np.inf)) | ((t2 > tmin) & (t2 < np.inf)))


def check_tables(spheres, scene, want_axes=None):
    """A list's window tables against the list: one record per segment, a table only on a run and on one of its varying axes;
    inside a windowed run every decided sphere lies inside the slab and inside its trip's span, and a trip with an undecided row has
    the span that is everything; outside, every span is everything."""
    segs = scene.scan_segments()
    wins, spans = scene.scan_windows()
    n = len(spheres)
    assert len(wins) == len(segs) and len(spans) == (n + TRIP - 1) // TRIP
    if want_axes is not None:
        assert [None if w is None else w[0] for w in wins] == want_axes, (wins, want_axes)
    dec = S.decided(spheres)
    everything = np.ones(len(spans), dtype=bool)
    for (first, rows, axis, _), win in zip(segs, wins):
        if win is None:
            continue
        assert axis is not None and win[0] != axis and win[0] in (0, 1, 2)
        for t in range(first // TRIP, (first + rows) // TRIP):
            everything[t] = False
            ks = [k for k in range(t * TRIP, min((t + 1) * TRIP, n))]
            lo, hi = float(spans[t, 0]), float(spans[t, 1])
            if any(not dec[k] for k in ks):
                assert lo == -np.inf and hi == np.inf, (t, lo, hi)
            for k in ks:
                if dec[k]:
                    (c, r) = spheres[k]
                    assert win[1] <= c[axis] - r and c[axis] + r <= win[2], (k, win)
                    assert lo <= c[win[0]] - r and c[win[0]] + r <= hi, (k, lo, hi)
    assert np.all(spans[everything, 0] == -np.inf) and np.all(spans[everything, 1] == np.inf)
    return segs, wins, spans
