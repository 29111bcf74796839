"""The segments of the sphere-list scan (csrc/scene_builder.cpp cut_scan_segments) through rt_scene_dump_scan_segments, without a
GPU: where the packed filter's loop runs its shared-coordinate form (render.hip filter_pairs<true>) and where the general one.

A run segment is a maximal range of whole trips (eight rows) whose decided rows share one fp32 centre coordinate bit for bit;
rows the fp32 filter does not decide (the ground sphere: far outside the bulk of the list) and the padding behind the list fit
any run; runs of fewer than four trips stay general.  The lists below place runs against every one of those rules, and
tests/test_list_scan_runs_gpu.py renders the same lists.
"""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from scan_segment_lists import CASES, GROUND, check_segments, decided, field, product


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_lists(name):
    spheres, want = CASES[name]
    segs = product(spheres).scan_segments()
    print(name, segs)
    check_segments(spheres, segs)
    assert [(f, r, a, float(c)) for f, r, a, c in segs] == want


def test_the_giant_is_undecided_and_the_rest_decided():
    for name, (spheres, _) in CASES.items():
        dec = decided(spheres)
        assert [k for k in range(len(spheres)) if not dec[k]] == [k for k, s in enumerate(spheres) if s == GROUND], name
    assert sum(GROUND in s for s, _ in CASES.values()) == 1


def test_signed_zeros_are_different_coordinates():
    """Bit-same, not equal: rows at y = +0 and y = -0 do not make one run."""
    rnd = np.random.default_rng(3)
    plus, minus = field(rnd, 16, y=0.0), field(rnd, 16, y=-0.0)
    assert product(plus + minus).scan_segments() == [(0, 32, None, 0.0)]
    segs = product(plus + field(rnd, 16, y=0.0)).scan_segments()
    assert [(f, r, a) for f, r, a, _ in segs] == [(0, 32, 1)] and np.float32(segs[0][3]).view(np.uint32) == 0


def test_an_empty_world_has_no_segments():
    assert product([]).scan_segments() == []


def test_benchmark_scene_is_one_run_on_y_and_a_last_general_trip():
    """Scene 11 as a list (config C2): the ground sphere in row 0 is undecided, rows 1 .. 481 rest on the plane at y = 0.2, and the
    three large spheres at y = 1 fall in the last trip."""
    s = rt.builtin_scene(11, 1, 1200, 800)
    segs = s.scan_segments()
    assert [(f, r, a) for f, r, a, _ in segs] == [(0, 480, 1), (480, 8, None)]
    assert np.float32(segs[0][3]).view(np.uint32) == np.float32(0.2).view(np.uint32)
