"""Light sampling queries on the device (rt_scene_sample_lights, rt_scene_light_pdf; Scene.sample_lights, Scene.light_pdf).  The
strict build against the numpy restatement (tests/light_restated.py) bit for bit; the sampled directions against the library's own
ray queries; the density call against the sampling call; and what it is all for: next-event estimation and multiple importance
sampling built from path_step + sample_lights + occluded agree in the mean with Scene.radiance."""
import functools
import math

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib

import light_restated as lr
from light_worlds import QUAD, TRIANGLE, SPHERE, MSPHERE, free_points, many_lights_world, mixed_world, no_lights_world, single_kind_world

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COUNTS = (1, 63, 64, 65, 257)
N = max(COUNTS)
SEED = 77
OUTPUTS = tuple(_lib.LIGHT_SAMPLE_OUTPUTS)
CAP = _lib.light_lds_rows()

WORLDS = {
    "quads": lambda: single_kind_world(QUAD), "triangles": lambda: single_kind_world(TRIANGLE), "spheres": lambda: single_kind_world(SPHERE),
    "moving spheres": lambda: single_kind_world(MSPHERE), "mixed": lambda: mixed_world()[::2],
    "cap": lambda: many_lights_world(CAP), "cap + 1": lambda: many_lights_world(CAP + 1),
}


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype.itemsize == 4 else a


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def inputs():
    arrays = free_points(N) + (lr.seeded_states(N, SEED),)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def restated(name, strategy):
    """The restatement of N samples in the world, from the library's own table: computed once, shared, read-only."""
    s, emission = world(name)
    P, nrm, mat, tm, states = inputs()
    out = lr.sample_lights(s.lights(), P, states, strategy=strategy, normals=nrm, materials=mat, times=tm, emission=emission)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- 1. the strict build is the restatement, bit for bit ----
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_strict_samples_are_the_restatement_bit_for_bit(name):
    s, _ = world(name)
    P, nrm, mat, tm, states = inputs()
    assert s.info()["n_lights"] == {"cap": CAP, "cap + 1": CAP + 1}.get(name, s.info()["n_lights"])
    for strategy in (0, 1):
        want = restated(name, strategy)
        assert want["valid"].mean() > 0.5, "the inputs exercise the sampling"
        for count in COUNTS:
            got = s.sample_lights(P[:count], nrm[:count], mat[:count], tm[:count], states[:count], strategy=strategy, variant=0, want=OUTPUTS)
            for key in OUTPUTS:
                assert np.array_equal(bits(got[key]), bits(want[key][:count])), (name, strategy, count, key)
    picked = set(restated(name, 0)["light"])
    assert len(picked) > 1 and (name not in ("cap + 1",) or max(picked) >= CAP - 8), "rows on both sides of the staged part are picked"


def test_a_row_beyond_the_staged_part_is_sampled_bit_for_bit():
    """Every point draws the same xi close to 1: the last row of the table of CAP + 1 lights, which no workgroup stages."""
    s, emission = world("cap + 1")
    P, nrm, mat, tm, _ = inputs()
    states = lr.seeded_states(4096, SEED + 1)
    first = lr.Streams(states).uniform()
    states = np.ascontiguousarray(states[first > 1.0 - 0.5 / (CAP + 1)][:8])
    assert len(states) >= 2
    n = len(states)
    want = lr.sample_lights(s.lights(), P[:n], states, normals=nrm[:n], materials=mat[:n], emission=emission)
    assert np.all(want["light"] == CAP)
    got = s.sample_lights(P[:n], nrm[:n], mat[:n], None, states, want=OUTPUTS)
    for key in OUTPUTS:
        assert np.array_equal(bits(got[key]), bits(want[key])), key


def test_seeded_streams_and_statistics():
    s, emission = world("mixed")
    P, nrm, mat, tm, states = inputs()
    want = restated("mixed", 1)
    got, st = s.sample_lights(P, nrm, mat, tm, None, strategy=1, seed=SEED, want=OUTPUTS, stats=True)   # curand_init(seed, k, 0) in the kernel
    for key in OUTPUTS:
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert (st.points, st.valid) == (N, int(want["valid"].sum())) and st.kernel_vgprs > 0 and st.seconds > 0.0
    later = s.sample_lights(P[:65], times=tm[:65], seed=SEED, first_sequence=100, strategy=1, want=("rng_state", "light"))
    assert np.array_equal(later["light"], lr.sample_lights(s.lights(), P[:65], lr.seeded_states(65, SEED, 100), strategy=1, times=tm[:65])["light"])
    _, st = s.light_pdf(P, np.ascontiguousarray(want["direction"] + (~want["valid"])[:, None] * np.array([0.0, -1.0, 0.0])), tm, strategy=1, stats=True)
    assert st.points == N and 0 < st.valid <= N and st.kernel_vgprs > 0


@pytest.mark.parametrize("variant", [0, 1])
def test_torch_and_numpy_paths_give_the_same_bits(variant):
    s, _ = world("mixed")
    P, nrm, mat, tm, states = inputs()
    for count in COUNTS:
        host = s.sample_lights(P[:count], nrm[:count], mat[:count], tm[:count], states[:count], strategy=1, variant=variant, want=OUTPUTS)
        dev = [torch.from_numpy(np.array(a[:count])).cuda() for a in (P, nrm, mat, tm)]
        stream = torch.from_numpy(states[:count].view(np.int32).copy()).cuda()
        got = s.sample_lights(*dev, stream, strategy=1, variant=variant, want=OUTPUTS, out={"rng_state": stream})   # the stream in place
        torch.cuda.synchronize()
        assert got["rng_state"].data_ptr() == stream.data_ptr()
        for key in OUTPUTS:
            assert np.array_equal(bits(got[key]), bits(host[key])), (count, key)
        pdf_host = s.light_pdf(P[:count], np.ascontiguousarray(host["direction"]), tm[:count], strategy=1, variant=variant, want=("pdf", "light"))
        pdf_dev = s.light_pdf(dev[0], got["direction"], dev[3], strategy=1, variant=variant, want=("pdf", "light"))
        for key in ("pdf", "light"):
            assert np.array_equal(bits(pdf_dev[key]), bits(pdf_host[key])), (count, key)


def test_a_scene_without_lights():
    s = no_lights_world()
    P, nrm, mat, tm, states = inputs()
    got = s.sample_lights(P[:65], nrm[:65], mat[:65], None, states[:65], want=OUTPUTS)
    assert np.all(got["light"] == -1) and np.array_equal(got["rng_state"], states[:65])
    for key in ("direction", "distance", "pdf", "emitted", "scatter_pdf", "contribution"):
        assert not got[key].any(), key
    assert np.array_equal(s.sample_lights(P[:65], seed=SEED, want=("rng_state",))["rng_state"], states[:65])   # seeded, then unchanged
    out = s.light_pdf(P[:65], np.tile([0.0, 1.0, 0.0], (65, 1)), want=("pdf", "light"))
    assert not out["pdf"].any() and np.all(out["light"] == -1)


# ---- 2. the sampled direction meets the sampled light ----
def inner_points(count):
    """Exactly ``count`` points like free_points', from which no lamp of a single-kind world stands in front of the other:
    |x|, |z| <= 1 below the lamps."""
    P, nrm, mat, tm = free_points(8 * count + 64, seed=11)
    keep = (np.abs(P[:, 0]) <= 1.0) & (np.abs(P[:, 2]) <= 1.0)
    out = tuple(np.ascontiguousarray(a[keep][:count]) for a in (P, nrm, mat, tm))
    assert len(out[0]) == count
    return out


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("kind", [QUAD, TRIANGLE, SPHERE, MSPHERE], ids=["quads", "triangles", "spheres", "moving spheres"])
def test_intersect_along_the_sampled_direction_finds_the_light(kind, variant):
    """``intersect`` from the point along ``direction`` reports the sampled light's leaf at t within 64 eps x distance of ``distance``.
    The bound: the sample S, D = S - P, its length and the unit direction are some ten roundings of values no larger than |P| + |S|
    <= 3.5 distance here (the lamps are at least one unit away, nothing lies further than 3.5 from the origin); the query's own t
    is another ten on the same magnitudes.  Twenty roundings of half an ulp of 3.5 distance: 35 eps x distance, under 64.  That
    count holds for the planar lamps.  A sphere's near root is ill-conditioned towards the cone's rim (its error grows like
    1 / sqrt(disc)), where no count of roundings bounds the difference between two ways of computing it: there the sampled
    distance IS the renderer's own root for the ray (point, direction) -- the sphere test's operations on the same operands -- so
    the query's t is the distance itself, not merely close to it."""
    s, _ = single_kind_world(kind)
    P, nrm, mat, tm = inner_points(257)
    L = s.lights()
    for strategy in (0, 1):
        got = s.sample_lights(P, nrm, mat, tm, None, seed=SEED + strategy, strategy=strategy, variant=variant)
        v = got["pdf"] > 0.0
        assert v.mean() > 0.9
        hit = s.intersect(P[v], np.ascontiguousarray(got["direction"][v]), times=tm[v], variant=variant, want=("t", "leaf", "material"))
        assert np.array_equal(hit["leaf"], L["leaf"][got["light"][v]]) and np.all(hit["material"] == 3)
        print("kind", kind, "variant", variant, "strategy", strategy, "max |t - distance| / (eps distance):",
              float(np.max(np.abs(hit["t"] - got["distance"][v]) / (EPS * got["distance"][v]))))
        assert np.all(np.abs(hit["t"] - got["distance"][v]) <= 64.0 * EPS * got["distance"][v])
        assert np.all(np.abs(np.sqrt((got["direction"][v] ** 2).sum(axis=1)) - 1.0) <= 4.0 * EPS)


# ---- 3. the density call against the sampling call ----
@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("kind", [QUAD, TRIANGLE], ids=["quads", "triangles"])
def test_light_pdf_along_a_sampled_direction_planar(kind, variant):
    s, _ = single_kind_world(kind)
    P, nrm, mat, tm = inner_points(257)
    L = s.lights()
    for strategy in (0, 1):
        got = s.sample_lights(P, nrm, mat, tm, None, seed=SEED, strategy=strategy, variant=variant)
        cos = np.abs((L["n"][got["light"]] * got["direction"]).sum(axis=1))
        assert np.all(got["pdf"] > 0.0) and cos.min() >= 0.05, "the points keep the lamps well off grazing"
        out = s.light_pdf(P, np.ascontiguousarray(got["direction"]), strategy=strategy, variant=variant, want=("pdf", "light"))
        assert np.array_equal(out["light"], got["light"])
        assert np.all(np.abs(out["pdf"] - got["pdf"]) <= (64.0 * EPS / cos) * got["pdf"])
        scaled = s.light_pdf(P, np.ascontiguousarray(4.0 * got["direction"]), strategy=strategy, variant=variant)["pdf"]   # not a unit vector
        assert np.all(np.abs(scaled - got["pdf"]) <= (64.0 * EPS / cos) * got["pdf"])


@pytest.mark.parametrize("kind", [SPHERE, MSPHERE], ids=["spheres", "moving spheres"])
def test_light_pdf_along_a_sampled_direction_spheres_strict(kind):
    """Bit for bit: the density of a sphere depends on the point alone.  Left out: the samples within 1e-12 of the cone's rim, where
    the density call's own hit test may miss the sphere; the restatement confirms that they are at most 1 % of these inputs."""
    s, emission = single_kind_world(kind)
    P, nrm, mat, tm = inner_points(257)
    n = len(P)
    for strategy in (0, 1):
        states = lr.seeded_states(n, SEED + 2)
        want = lr.sample_lights(s.lights(), P, states, strategy=strategy, times=tm)
        assert want["valid"].all() and want["rim"].mean() <= 0.01
        got = s.sample_lights(P, None, None, tm, states, strategy=strategy, want=("direction", "pdf", "light"))
        out = s.light_pdf(P, np.ascontiguousarray(got["direction"]), tm, strategy=strategy, want=("pdf", "light"))
        keep = ~want["rim"]
        assert np.array_equal(bits(out["pdf"][keep]), bits(got["pdf"][keep])) and np.array_equal(out["light"][keep], got["light"][keep])
        ref_pdf, ref_light = lr.light_pdf(s.lights(), P, got["direction"], strategy=strategy, times=tm)
        assert np.array_equal(bits(out["pdf"]), bits(ref_pdf)) and np.array_equal(out["light"], ref_light)


@pytest.mark.parametrize("name", ["cap", "cap + 1", "mixed"])
def test_light_pdf_is_the_restatement_bit_for_bit_on_both_sides_of_the_cap(name):
    """The density call's loop over all rows -- the staged ones and, with CAP + 1 lamps, the one it reads from global memory --
    against the restatement, strict build, for every count: along the sampled directions (the rays meet lamps, often several of
    the mesh's) and along directions of their own."""
    s, _ = world(name)
    P, nrm, mat, tm, _ = inputs()
    for strategy in (0, 1):
        d = np.where(restated(name, strategy)["valid"][:, None], restated(name, strategy)["direction"], nrm)
        d = np.ascontiguousarray(np.concatenate([d[::2], 3.0 * nrm[1::2]]))   # (not all unit vectors)
        Q, t = np.ascontiguousarray(np.concatenate([P[::2], P[1::2]])), np.ascontiguousarray(np.concatenate([tm[::2], tm[1::2]]))
        want_pdf, want_light = lr.light_pdf(s.lights(), Q, d, strategy=strategy, times=t)
        assert (want_light >= 0).mean() > 0.3 and (want_light < 0).any()
        if name == "cap + 1":   # the row beyond the staged part is met too: aim a few rays at its middle
            L = s.lights()
            Q = np.ascontiguousarray(Q.copy())
            d = np.ascontiguousarray(d.copy())
            d[:4] = (L["a"][CAP] + 0.5 * L["b"][CAP] + 0.5 * L["c"][CAP]) - Q[:4]
            want_pdf, want_light = lr.light_pdf(L, Q, d, strategy=strategy, times=t)
            assert np.all(want_light[:4] == CAP)
        for count in COUNTS:
            got = s.light_pdf(Q[:count], d[:count], t[:count], strategy=strategy, variant=0, want=("pdf", "light"))
            assert np.array_equal(bits(got["pdf"]), bits(want_pdf[:count])) and np.array_equal(got["light"], want_light[:count]), (strategy, count)


def test_light_pdf_sums_overlapping_lights_and_misses_give_zero():
    s = rt.Scene()
    lamp = s.DiffuseLight((4, 4, 4))
    s.SetWorld(s.HittableList([s.Quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), lamp), s.Quad((-3, 3, -3), (6, 0, 0), (0, 0, 6), lamp),
                               s.Sphere((0, 6, 0), 1.0, lamp)]))
    s.Camera((0, 0, 10), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, background=(0, 0, 0))
    s.Commit()
    g = np.random.default_rng(5)
    P = np.ascontiguousarray(g.uniform(-0.25, 0.25, size=(65, 3)))
    target = np.ascontiguousarray(g.uniform((-0.9, 2.0, -0.9), (0.9, 2.0, 0.9), size=(65, 3)))
    d = np.ascontiguousarray(target - P)
    for strategy in (0, 1):
        cdf = s.lights()["cdf"][:, strategy]
        chance = np.diff(np.concatenate([[0.0], cdf]))
        out = s.light_pdf(P, d, strategy=strategy, want=("pdf", "light"))
        assert np.all(out["light"] == 0)
        unit = d / np.linalg.norm(d, axis=1, keepdims=True)
        want = np.zeros(65)
        for k, (height, area) in enumerate(((2.0, 4.0), (3.0, 36.0))):
            dist = (height - P[:, 1]) / unit[:, 1]
            want += dist * dist / (unit[:, 1] * area) * chance[k]
        oc = np.array([0.0, 6.0, 0.0]) - P
        b = (oc * unit).sum(axis=1)
        disc = b * b - ((oc * oc).sum(axis=1) - 1.0)
        hits_sphere = disc > 0.0
        assert np.all(np.abs(disc) > 1e-6) and hits_sphere.any() and not hits_sphere.all()   # (no ray grazes it)
        want += hits_sphere * chance[2] / (2.0 * math.pi * (1.0 - np.sqrt(1.0 - 1.0 / (oc * oc).sum(axis=1))))
        assert np.all(np.abs(out["pdf"] - want) <= 1e-12 * want)
        ref_pdf, ref_light = lr.light_pdf(s.lights(), P, d, strategy=strategy)
        assert np.array_equal(bits(out["pdf"]), bits(ref_pdf)) and np.array_equal(out["light"], ref_light)
        away = s.light_pdf(P, np.ascontiguousarray(-d), strategy=strategy, want=("pdf", "light"))
        assert not away["pdf"].any() and np.all(away["light"] == -1)


# ---- 4. the point of it all ----
BATCHES = 16
SAMPLES = 4096   # per point and batch: 65 536 a point in all, which brings the lit points' combined standard error under 2 % of their mean
LAMP = ((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
BALL = ((1.2, 1.5, 0.3), 0.25)
SHADE = ((-0.1, 0.5, -0.4), (1.0, 0.0, 0.0), (0.0, 0.0, 0.8))


def lamp_scene():
    s = rt.Scene()
    floor = s.Lambertian(s.CheckerTexture(0.5, s.SolidColor((0.8, 0.8, 0.8)), s.SolidColor((0.3, 0.5, 0.7))))
    s.SetWorld(s.HittableList([s.Quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), floor), s.Quad(*LAMP, s.DiffuseLight((8.0, 8.0, 8.0))),
                               s.Sphere(*BALL, s.DiffuseLight((10.0, 6.0, 3.0))), s.Quad(*SHADE, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 1, 6), (0, 1, 0), (0, 1, 0), 40.0, 1.0, 0.0, 6.0, background=(0, 0, 0))
    s.Commit()
    return s


def in_full_shadow(p):
    """Sufficient: the lamp's corners and the corners of the ball's bounding box, seen from the floor point, all fall inside the shade
    where their rays cross its plane (the shade is convex, so does everything between them)."""
    corners = [np.array(LAMP[0]) + a * np.array(LAMP[1]) + b * np.array(LAMP[2]) for a in (0, 1) for b in (0, 1)]
    corners += [np.array(BALL[0]) + BALL[1] * np.array([a, b, c]) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    for c in corners:
        x = p + (SHADE[0][1] - p[1]) / (c[1] - p[1]) * (c - p)
        if not (SHADE[0][0] + 0.01 <= x[0] <= SHADE[0][0] + SHADE[1][0] - 0.01 and SHADE[0][2] + 0.01 <= x[2] <= SHADE[0][2] + SHADE[2][2] - 0.01):
            return False
    return True


def test_next_event_estimation_and_mis_agree_with_radiance():
    """A: Scene.radiance(max_depth=2).  B: path_step, sample_lights, occluded(*shadow_rays), attenuation * contribution * visible.
    C: both strategies combined by the balance heuristic through light_pdf and rt.scatter_pdf.  16 independent batches each give a
    standard error per point and channel; A - B and A - C stay within 5 combined standard errors everywhere, at 4096 samples a
    point and batch the lit points' combined standard error is under 2 % of their mean -- a cosine lobe in place of 2 cos^3 / pi
    would be off by up to a factor of 2 -- and a point in full shadow gets exactly nothing from B."""
    s = lamp_scene()
    xs = -1.4 + 0.4 * np.arange(8)
    o = np.ascontiguousarray(np.array([(x, 0.05, z) for x in xs for z in xs]))
    d = np.ascontiguousarray(np.tile([0.0, -1.0, 0.0], (64, 1)))
    shadowed = np.array([in_full_shadow(np.array([p[0], 0.0, p[2]])) for p in o])
    assert 2 <= shadowed.sum() <= 16
    A = np.stack([s.radiance(o, d, samples=SAMPLES, max_depth=2, seed=100, first_sequence=64 * b)["radiance"] for b in range(BATCHES)])
    O = torch.from_numpy(np.repeat(o, SAMPLES, axis=0)).cuda()
    D = torch.from_numpy(np.repeat(d, SAMPLES, axis=0)).cuda()
    n = O.shape[0]
    B, Cm = [], []
    for b in range(BATCHES):
        step = s.path_step(O, D, seed=200, first_sequence=n * b, want=("status", "attenuation", "origin", "direction", "normal", "material", "rng_state"))
        assert bool((step["status"] == 2).all())
        ls = s.sample_lights(step["origin"], step["normal"], step["material"], None, step["rng_state"])
        vis = ~s.occluded(*s.shadow_rays(step["origin"], ls["direction"], ls["distance"]))
        direct = step["attenuation"] * ls["contribution"] * vis[:, None]
        B.append(direct.reshape(64, SAMPLES, 3).mean(dim=1).cpu().numpy())
        # the same light samples weighted p_l / (p_l + p_s), and what the scattered ray finds weighted p_s / (p_s + p_l)
        p_l = s.light_pdf(step["origin"], ls["direction"])["pdf"]
        w_l = torch.where(p_l + ls["scatter_pdf"] > 0, p_l / (p_l + ls["scatter_pdf"]), torch.zeros_like(p_l))
        unit = step["direction"] / torch.linalg.norm(step["direction"], dim=1, keepdim=True)
        p_s = rt.scatter_pdf(step["material"], step["normal"], unit)
        q_l = s.light_pdf(step["origin"], step["direction"])["pdf"]
        found = s.path_step(step["origin"], step["direction"], rng_state=ls["rng_state"], want=("emitted",))["emitted"]
        w_s = torch.where(p_s > 0, p_s / (p_s + q_l), torch.zeros_like(p_s))
        mis = direct * w_l[:, None] + step["attenuation"] * found * w_s[:, None]
        Cm.append(mis.reshape(64, SAMPLES, 3).mean(dim=1).cpu().numpy())
    B, Cm = np.stack(B), np.stack(Cm)

    def mean_se(x):
        return x.mean(axis=0), x.std(axis=0, ddof=1) / math.sqrt(BATCHES)

    (a, sa), (bm, sb), (cm, sc) = mean_se(A), mean_se(B), mean_se(Cm)
    lit = a.sum(axis=1) > 0.0
    print("lit points", int(lit.sum()), "mean A", a[lit].mean(), "combined se A-B", np.sqrt(sa ** 2 + sb ** 2)[lit].mean(),
          "A-C", np.sqrt(sa ** 2 + sc ** 2)[lit].mean(), "max |A-B| / se", np.nanmax(np.abs(a - bm)[lit] / np.sqrt(sa ** 2 + sb ** 2)[lit]),
          "max |A-C| / se", np.nanmax(np.abs(a - cm)[lit] / np.sqrt(sa ** 2 + sc ** 2)[lit]))
    assert np.all(np.abs(a - bm) <= 5.0 * np.sqrt(sa ** 2 + sb ** 2))
    assert np.all(np.abs(a - cm) <= 5.0 * np.sqrt(sa ** 2 + sc ** 2))
    assert np.sqrt(sa ** 2 + sb ** 2)[lit].mean() <= 0.02 * a[lit].mean() and np.sqrt(sa ** 2 + sc ** 2)[lit].mean() <= 0.02 * a[lit].mean()
    assert lit.sum() >= 40 and not lit[shadowed].any()
    assert not B[:, shadowed].any(), "a point in full shadow gets exactly nothing from the light samples"
    assert np.abs(bm[lit] / a[lit] - 1.0).mean() < 0.05   # (and no factor of 2 anywhere near)
