"""Sphere lists placed against the rules that cut the sphere-list scan into segments (csrc/scene_builder.cpp cut_scan_segments),
with the segments each must give, and the checks both tests/test_scan_segments_host.py and tests/test_list_scan_runs_gpu.py make on
them.  Not a test module."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt

TRIP = 8        # rows per trip of the loop (render.hip kFilterTrip)
MIN_TRIPS = 4   # flat_scene.h kScanRunMinTrips
W, H = 64, 48
GROUND = ((0.0, -1000.5, -5.0), 1000.0)


def field(rnd, n, **fixed):
    """n small spheres in front of the camera, ((x, y, z), radius); x / y / z given: that coordinate is the same for all."""
    out = []
    for _ in range(n):
        c = [float(rnd.uniform(-3, 3)), float(rnd.uniform(-0.4, 1.2)), float(rnd.uniform(-9, -3))]
        for axis, name in enumerate("xyz"):
            if name in fixed:
                c[axis] = fixed[name]
        out.append((tuple(c), float(rnd.uniform(0.15, 0.45))))
    return out


def _cases():
    """name -> (spheres in list order, the segments they must give as (first_row, n_rows, axis, shared))."""
    rnd = np.random.default_rng(20261)
    f32 = lambda v: float(np.float32(v))
    cases = {}
    cases["no_run"] = (field(rnd, 40), [(0, 40, None, 0.0)])
    cases["one_trip_short"] = (field(rnd, 24, y=0.3) + field(rnd, 16), [(0, 40, None, 0.0)])
    cases["exactly_the_minimum"] = (field(rnd, 32, y=0.3) + field(rnd, 16), [(0, 32, 1, f32(0.3)), (32, 16, None, 0.0)])
    # rows 5 .. 44 share y: the whole trips among them are rows 8 .. 39
    cases["off_trip_boundaries"] = (field(rnd, 5) + field(rnd, 40, y=0.3) + field(rnd, 11),
                                    [(0, 8, None, 0.0), (8, 32, 1, f32(0.3)), (40, 16, None, 0.0)])
    giant = field(rnd, 48, y=0.3)
    giant[20] = GROUND
    cases["undecided_giant_inside"] = (giant, [(0, 48, 1, f32(0.3))])
    cases["two_axes_back_to_back"] = (field(rnd, 32, x=0.5) + field(rnd, 32, z=-6.0), [(0, 32, 0, f32(0.5)), (32, 32, 2, f32(-6.0))])
    cases["one_axis_two_values"] = (field(rnd, 32, y=0.3) + field(rnd, 32, y=0.9), [(0, 32, 1, f32(0.3)), (32, 32, 1, f32(0.9))])
    # 45 rows: the run's last trip ends in three rows of padding
    cases["up_to_the_padded_end"] = (field(rnd, 10) + field(rnd, 35, y=0.3), [(0, 16, None, 0.0), (16, 32, 1, f32(0.3))])
    return cases


CASES = _cases()


def _material(s, k):
    if k % 7 == 0:
        return s.Dielectric(1.5)
    if k % 3 == 0:
        return s.Metal((0.8, 0.6 + 0.03 * (k % 10), 0.5), 0.02 * (k % 8))
    return s.Lambertian((0.1 + 0.08 * (k % 10), 0.5, 0.9 - 0.07 * (k % 11)))


def world(spheres):
    """A build function for conftest.build_both / product(): the spheres as a HittableList in this order."""
    def build(s, Rng):
        items = [s.Sphere(c, r, _material(s, k)) for k, (c, r) in enumerate(spheres)]
        s.SetWorld(s.HittableList(items))
        s.Camera((0.0, 0.3, 0.5), (0.0, 0.0, -5.0), (0, 1, 0), 50, W / H, 0.0, 10.0)
        s.Commit()
    return build


def product(spheres):
    s = rt.Scene()
    world(spheres)(s, rt.Rng)
    return s


def decided(spheres):
    """Which rows the fp32 filter decides (scene_builder.cpp): those within four times the median of |centre| + radius.  This
    restates the host's rule for the lists of this file, where it is the only one that bites: a row with a non-finite k or a reach
    of 1e15 and more is undecided too, and none of these lists has one (test_the_giant_is_undecided_and_the_rest_decided pins which
    rows the rule leaves out here)."""
    reach = np.array([np.sqrt(np.dot(c, c)) + r for c, r in spheres])
    return reach <= 4.0 * np.sort(reach)[len(reach) // 2]


def check_segments(spheres, segs):
    """The segments tile the trips exactly and in order; every decided row of a run has the run's coordinate bit for bit; no run is
    shorter than the minimum."""
    n = len(spheres)
    trips = (n + TRIP - 1) // TRIP
    at = 0
    for first, rows, axis, shared in segs:
        assert first == at and rows > 0 and first % TRIP == 0 and rows % TRIP == 0, segs
        at += rows
        if axis is None:
            continue
        assert rows >= MIN_TRIPS * TRIP, segs
        dec = decided(spheres)
        for k in range(first, min(first + rows, n)):
            if dec[k]:
                assert np.float32(spheres[k][0][axis]).view(np.uint32) == np.float32(shared).view(np.uint32), (k, axis, shared)
    assert at == trips * TRIP, segs
