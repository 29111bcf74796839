"""What the sphere-list scan tests (kernel kind 16) share: the loose field of small spheres their worlds are made of, the frame
rendered twice -- SPP samples, then MORE continued from the saved RNG streams -- and the comparisons of two such renders and of
the strict build with the CPU oracle.  The worlds, the cases and what is particular to a feature stay in the test files."""
import collections

import numpy as np

import raytracinginoneweekendincuda_amd as rt

SPP, MORE = 4, 2

Scan = collections.namedtuple("Scan", "first continued rays more_rays kernel_kind pixels_per_wave")


def material(s, rnd, k):
    if k % 7 == 0:
        return s.Dielectric(1.5)
    if k % 3 == 0:
        return s.Metal(tuple(rnd.uniform(0.4, 0.9, 3)), float(rnd.uniform(0.0, 0.3)))
    return s.Lambertian(tuple(rnd.uniform(0.1, 0.9, 3)))


def small_spheres(s, rnd, n):
    """A loose field of small spheres in front of the camera (what the filter decides)."""
    items = []
    for k in range(n):
        c = (float(rnd.uniform(-3, 3)), float(rnd.uniform(-0.4, 1.2)), float(rnd.uniform(-9, -3)))
        items.append(s.Sphere(c, float(rnd.uniform(0.15, 0.45)), material(s, rnd, k)))
    return items


def ground(s):
    return s.Sphere((0.0, -1000.5, -5.0), 1000.0, s.Lambertian((0.5, 0.5, 0.5)))


def render_twice(prod, w, h, variant, flags, *, depth=None, film=None, render=None, adaptive=None):
    """SPP samples, then MORE from the saved RNG streams.  ``film`` and ``adaptive`` are the keywords of rt.Film and of
    Film.set_adaptive, ``render`` those of both launches (a forcing: coop_threshold, pixels_per_wave); ``depth`` None is the
    library's default."""
    f = rt.Film(w, h, **(film or {}))
    if adaptive is not None:
        f.set_adaptive(**adaptive)
    common = dict(variant=variant, **(render or {}))
    if depth is not None:
        common["max_depth"] = depth
    st = f.render(prod, SPP, flags=flags, **common)
    first = f.download().copy()
    st2 = f.render(prod, MORE, flags=flags | rt.FLAG_KEEP_RNG_STATE, **common)
    return Scan(first, f.download().copy(), st.rays, st2.rays, st.kernel_kind, st.pixels_per_wave)


def assert_same_scan(got, ref, label):
    """Both ray counts, the frame and the continued frame of two render_twice records, bit for bit."""
    assert got.rays == ref.rays and got.more_rays == ref.more_rays, (
        label, "ray counts differ", (got.rays, got.more_rays), (ref.rays, ref.more_rays))
    assert np.array_equal(got.first.view(np.uint64), ref.first.view(np.uint64)), label
    assert np.array_equal(got.continued.view(np.uint64), ref.continued.view(np.uint64)), (label, "continued streams")


def assert_strict_equals_oracle(got, want, stats, rows=None, label=None):
    """The strict build's first frame against the oracle's, bit for bit, on ``rows`` (None: the whole frame) -- and the oracle's
    ray count, where the rows are the whole frame."""
    if rows is None or len(rows) == len(want):
        assert got.rays == stats["rays"], label
    rows = slice(None) if rows is None else rows
    assert np.array_equal(got.first[rows].view(np.uint64), want[rows].view(np.uint64)), label
