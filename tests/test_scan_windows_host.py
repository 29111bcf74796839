"""The window rule of the sphere-list scan (csrc/scan_window_rule.h) against the reference's sphere test, without a device.

A pixel-parallel pass runs, of a run with a window table, only the trips the rule calls needed for some ray of the pass.  The rule
may call a trip needed in vain; it must never leave out a trip that holds a sphere the reference's Sphere::Hit accepts over
(0.001, inf).  rt_scene_scan_window_trips evaluates the rule for one ray at a time exactly as the kernel does (a pass's union of
rays and its filled gaps only ever add trips), and tests/scan_window_lists.py restates the reference's test in numpy: for every
ray of every kind below and every sphere of every list, an accepted sphere lies in a needed trip.
"""
import numpy as np
import pytest

import scan_segment_lists as S
import scan_window_lists as L

TRIP = L.TRIP


def rays_for(spheres, wins, segs, seed):
    """The rays of the issue's list, a few hundred of each kind, as (origins, directions, kind per ray)."""
    rnd = np.random.default_rng(seed)
    c = np.array([s[0] for s in spheres])
    r = np.array([s[1] for s in spheres])
    small = r < 10.0
    lo, hi = (c - r[:, None])[small].min(0), (c + r[:, None])[small].max(0)
    mid, ext = 0.5 * (lo + hi), (hi - lo) + 1.0
    runs = [(axis, win) for (_, _, axis, _), win in zip(segs, wins) if win is not None] or [(1, (0, lo[1], hi[1]))]
    os_, ds_, kinds = [], [], []

    def add(kind, o, d):
        os_.append(np.asarray(o, dtype=np.float64).reshape(-1, 3))
        ds_.append(np.asarray(d, dtype=np.float64).reshape(-1, 3))
        kinds.extend([kind] * len(os_[-1]))

    n = 400
    add("random", mid + rnd.uniform(-1.0, 1.0, (n, 3)) * ext, rnd.normal(size=(n, 3)))
    picks = rnd.integers(0, len(spheres), n)
    o = mid + rnd.uniform(-1.0, 1.0, (n, 3)) * ext
    add("at a sphere", o, (c[picks] + rnd.normal(size=(n, 3)) * r[picks, None] * 0.7 - o) * rnd.uniform(0.2, 3.0, (n, 1)))
    for axis, win in runs:
        w_axis, s_lo, s_hi = int(win[0]), float(win[1]), float(win[2])
        # d[axis] = 0 exactly, the origin inside and outside the slab
        o = mid + rnd.uniform(-1.0, 1.0, (n, 3)) * ext
        o[: n // 2, axis] = rnd.uniform(s_lo, s_hi, n // 2)
        o[n // 2:, axis] = np.where(rnd.random(n - n // 2) < 0.5, s_lo - rnd.uniform(1e-9, 2.0, n - n // 2), s_hi + rnd.uniform(1e-9, 2.0, n - n // 2))
        d = rnd.normal(size=(n, 3))
        d[:, axis] = 0.0
        add("parallel to the slab", o, d)
        # origins inside the slab, and inside spheres
        o = mid + rnd.uniform(-1.0, 1.0, (n, 3)) * ext
        o[:, axis] = rnd.uniform(s_lo, s_hi, n)
        add("from inside the slab", o, rnd.normal(size=(n, 3)))
        picks = rnd.integers(0, len(spheres), n)
        add("from inside a sphere", c[picks] + rnd.uniform(-0.55, 0.55, (n, 3)) * r[picks, None], rnd.normal(size=(n, 3)))
        # no component on the window axis
        d = rnd.normal(size=(n, 3))
        d[:, w_axis] = 0.0
        o = c[picks] + rnd.uniform(-1.5, 1.5, (n, 3)) * r[picks, None]
        o[:, axis] += rnd.uniform(-3.0, 3.0, n)
        add("along the window's planes", o, d)
    # tangents that graze a sphere by +-1e-12 relative (and by nothing, and by a little more)
    picks = rnd.integers(0, len(spheres), 2 * n)
    far = rnd.choice([1.0, 1.0, 10.0], 2 * n)
    o = mid + rnd.uniform(-1.0, 1.0, (2 * n, 3)) * ext * far[:, None]
    perp = np.cross(c[picks] - o, rnd.normal(size=(2 * n, 3)))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    eps = rnd.choice([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, -1e-3], 2 * n)
    d = (c[picks] + perp * (r[picks] * (1.0 + eps))[:, None] - o) * rnd.uniform(0.2, 3.0, (2 * n, 1)) * rnd.choice([1.0, -1.0], (2 * n, 1))
    add("grazing", o, d)
    # origins at 1e6, aimed at the spheres
    picks = rnd.integers(0, len(spheres), n)
    o = rnd.normal(size=(n, 3))
    o *= 1e6 / np.linalg.norm(o, axis=1)[:, None]
    add("from 1e6", o, (c[picks] + rnd.normal(size=(n, 3)) * r[picks, None] * 0.5 - o) * rnd.uniform(0.5, 2.0, (n, 1)))
    # degenerate directions
    o = mid + rnd.uniform(-1.0, 1.0, (40, 3)) * ext
    add("zero direction", o, np.zeros((40, 3)))
    add("1e300 direction", o, rnd.normal(size=(40, 3)) * 1e300)
    return np.concatenate(os_), np.concatenate(ds_), np.array(kinds)


def assert_rule_covers_the_reference(scene, spheres, seed, want_axes=None):
    segs, wins, spans = L.check_tables(spheres, scene, want_axes)
    o, d, kinds = rays_for(spheres, wins, segs, seed)
    need = scene.scan_window_trips(o, d)
    assert need.shape == (len(o), len(spans))
    accepted = L.reference_accepts(o, d, spheres)
    trip_of = np.arange(len(spheres)) // TRIP
    missed = accepted & ~need[:, trip_of]
    assert not missed.any(), [(kinds[i], o[i].tolist(), d[i].tolist(), int(k)) for i, k in zip(*np.nonzero(missed))][:5]
    windowed = np.zeros(len(spans), dtype=bool)
    for (first, rows, _, _), win in zip(segs, wins):
        if win is not None:
            windowed[first // TRIP:(first + rows) // TRIP] = True
    assert need[:, ~windowed].all(), "a trip outside the windowed runs always runs"
    degenerate = np.isin(kinds, ("zero direction", "1e300 direction"))
    assert need[degenerate].all(), "a degenerate ray needs every trip"
    return need, accepted, kinds, windowed


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_no_accepted_sphere_lies_in_a_trip_the_rule_leaves_out(name):
    spheres, want_axes = L.CASES[name]
    scene = S.product(spheres)
    need, accepted, kinds, windowed = assert_rule_covers_the_reference(scene, spheres, sorted(L.CASES).index(name), want_axes)
    # the check has teeth: rays of every kind are accepted somewhere, and where a list has a table the rule does leave trips out
    for kind in ("random", "at a sphere", "grazing", "from 1e6"):
        assert accepted[kinds == kind].any(), kind
    if windowed.any():
        for kind in ("parallel to the slab", "from inside the slab", "from inside a sphere", "along the window's planes"):
            assert accepted[kinds == kind].any(), kind
        assert need[:, windowed].mean() < 0.6, "the windows are not selective for these rays"
    else:
        assert need.all()


def test_scene_11_has_a_window_on_x_and_the_rule_covers_the_reference():
    """Config C2's list: the run on y = 0.2 is stored x-cell major, so its trips are narrow on x (and wide on z); the ground
    sphere's trip and the last, general trip always run."""
    scene, spheres = L.scene11()
    need, accepted, kinds, windowed = assert_rule_covers_the_reference(scene, spheres, 11, [0, None])
    assert windowed.sum() == 60 and not windowed[60]
    assert need[:, 0].all(), "the ground sphere is undecided: its trip always runs"
    segs, wins, spans = L.check_tables(spheres, scene)
    assert wins[0][1] <= 0.0 and wins[0][2] >= 0.4 and wins[0][2] < 0.41, wins[0]
    widths = spans[1:60, 1] - spans[1:60, 0]
    assert widths.max() < 3.0, "a trip of 8 rows covers at most two cells of x and the radii"


@pytest.mark.parametrize("step,has_table", [(1.01, True), (0.99, False)])
def test_a_run_gets_a_table_from_a_quarter_on(step, has_table):
    """Mean span / extent = 1 / (3 step + 1): just under a quarter at step 1.01 (a table, on x), just over at 0.99 (none)."""
    spheres = L.quarter(step)
    scene = S.product(spheres)
    assert [(f, r, a) for f, r, a, _ in scene.scan_segments()] == [(0, 32, 1)]
    ratio = (1.0) / (3.0 * step + 1.0)
    assert (ratio <= L.MAX_MEAN_SPAN) == has_table
    wins, _ = scene.scan_windows()
    assert (wins[0] is not None) == has_table
    if has_table:
        assert wins[0][0] == 0
    assert_rule_covers_the_reference(scene, spheres, 5)


def test_a_list_without_a_run_has_no_tables():
    spheres, _ = S.CASES["no_run"]
    scene = S.product(spheres)
    wins, spans = scene.scan_windows()
    assert wins == [None] and np.all(spans[:, 0] == -np.inf) and np.all(spans[:, 1] == np.inf)
    o = np.zeros((3, 3))
    d = np.eye(3)
    assert scene.scan_window_trips(o, d).all()


def test_the_spans_are_staged_in_lds_with_the_sphere_planes():
    """rt_plan_launch: the spans lie behind the packed rows, 8 bytes a trip (C2: 61 trips); a list whose planes do not fit LDS reads
    them from global memory; a list without a windowed run has no such table and its block is what it was."""
    from frame_helpers import render_params
    scene, _ = L.scene11()
    pl = scene.plan_launch(render_params(1200, 800, 500))
    pairs, spans = pl["lds_tables"]["scan_pairs"], pl["lds_tables"]["scan_spans"]
    assert pl["kernel_kind"] == 16 and pl["lds_spheres"] == 1
    assert spans == (pairs[0] + pairs[1], 61 * 8) and spans[0] % 16 == 0 and pl["lds_bytes"] == spans[0] + spans[1] <= 52 * 1024
    rnd = np.random.default_rng(3)
    over = S.product(S.field(rnd, 16) + L.row(rnd, 1220 - 16, 1, 0.3, 0, -40.0, 40.0, radius=(0.05, 0.12)))
    pl = over.plan_launch(render_params(64, 48, 4))
    assert pl["lds_spheres"] == 0 and pl["lds_tables"]["scan_spans"] == (None, 153 * 8)
    none = S.product(S.CASES["no_run"][0])
    pl = none.plan_launch(render_params(64, 48, 4))
    assert pl["lds_tables"]["scan_spans"] == (None, 0) and pl["lds_bytes"] == pl["lds_tables"]["scan_pairs"][0] + pl["lds_tables"]["scan_pairs"][1]
