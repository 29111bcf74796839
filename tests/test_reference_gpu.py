"""Rays off the camera against the reference's own classes: Scene.intersect, Scene.occluded, Scene.path_step, Scene.radiance and
PathBatch.run of the strict build against what Hittable::Hit, Material::Scatter and Emitted of the reference, compiled for the host,
answered for the same rays, windows, times and streams.  Reads tests/golden/reference_hits.npz and nothing else of the reference
(tests/golden/make_reference_golden.py wrote it; tests/reference_worlds.py has the worlds and the file's layout).  Three worlds in
both world kinds, five sets of 512 rays each: origins inside glass, boxes and media, directions with exact zeros, directions of
length 1e-3 and 1e3, windows around the reference's own T, times outside the movers' interval."""
import functools
import os

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import reference_worlds as RW
from conftest import ROOT
from query_helpers import bits, uv_bound

pytestmark = pytest.mark.gpu

CASES = [(name, kind) for name in RW.WORLDS for kind in RW.KINDS]
IDS = [f"{name}-{('bvh', 'list')[kind]}" for name, kind in CASES]
# A ray that ends inside a medium has T = T1 + (negInvDensity * log(u)) / length (R/ConstantMedium.h:79,86): the device's log may
# differ from glibc's by an ulp, which passes through one multiply, one divide and one add on values of T's own size.
MEDIUM_REL = 8 * 2.0 ** -52
# What a NoiseTexture's colour may differ by: the device's sin against glibc's under 0.5 * (1 + sin(..)); the absolute tolerance the
# shading tests allow a pixel of such a texture (tests/frame_helpers.py:7-9, applied by tests/test_shading_gpu.py check()).
NOISE_ABS = 1e-5


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_hits.npz")) as g:
        return RW.Fixture({k: g[k] for k in g.files})


@functools.lru_cache(maxsize=None)
def scene_of(name, kind):
    return RW.build(name, rt.Scene(), rt.Rng, kind)


def describe(k, o, d, time, tmin, tmax):
    return f"ray {k}: origin {o[k].tolist()} direction {d[k].tolist()} time {time[k]!r} window ({tmin[k]!r}, {tmax[k]!r})"


def medium_report(label, got_t, want_t):
    """Prints the worst relative difference and the bit-exact share of t over the rays a medium had a say in; returns the worst."""
    if len(want_t) == 0:
        return 0.0
    rel = np.abs(got_t - want_t) / np.abs(want_t)
    exact = float(np.mean(bits(got_t) == bits(want_t)))
    print(f"{label}: {len(want_t)} rays, worst relative difference of t {rel.max():.3g} (bound {MEDIUM_REL:.3g}), bit-exact {exact:.4f}")
    return float(rel.max())


# ---- Scene.intersect and Scene.occluded ----
@pytest.mark.parametrize("set_name", RW.SETS)
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_closest_hits_are_the_references(name, kind, set_name):
    fx, scene = fixture(), scene_of(name, kind)
    o, d, time, tmin, tmax = fx.rays(name, set_name)
    want = fx.hits(name, kind, set_name)
    got = scene.intersect(o, d, times=time, tmin=tmin, tmax=tmax, seed=RW.SEED, variant=0, want=("t", "normal", "uv", "front_face", "material"))
    hit = np.isfinite(got["t"])
    # no ray is left out of the decisions: a flip against the reference in the strict build is a finding
    flips = np.flatnonzero(hit != (want["hit"] != 0))
    assert len(flips) == 0, f"{len(flips)} hit decisions differ; the reference {'hits' if want['hit'][flips[0]] else 'misses'}: " + describe(flips[0], o, d, time, tmin, tmax)
    for key in ("front_face", "material"):
        wrong = np.flatnonzero(got[key] != want[key])
        assert len(wrong) == 0, f"{key}: {got[key][wrong[0]]} != {want[key][wrong[0]]}: " + describe(wrong[0], o, d, time, tmin, tmax)
    surface = want["shape"] <= 1
    # the query stores 0 + normal, as the feature pass stores its sample (csrc/render.hip query_kernel: "no negative zeros"): the back
    # of a quad whose normal is (-1, +0, +0) is (1, -0, -0) in the reference's record and (1, 0, 0) here -- every other bit is compared
    for key, w in (("t", want["t"]), ("normal", want["normal"] + 0.0)):
        wrong = np.flatnonzero(surface & np.any((bits(got[key]) != bits(w)).reshape(len(o), -1), axis=-1))
        assert len(wrong) == 0, f"{key}: {got[key][wrong[0]]!r} != {w[wrong[0]]!r}: " + describe(wrong[0], o, d, time, tmin, tmax)
    flat = want["shape"] == 1      # quads and box faces: alpha, beta are sums and products
    assert np.array_equal(bits(got["uv"][flat]), bits(want["uv"][flat]))
    ball = want["shape"] == 0      # spheres: acos, atan2 of the (bit-identical) outward normal
    err = np.abs(got["uv"][ball] - want["uv"][ball])
    assert np.all(err <= uv_bound(want["normal"][ball]))
    fog = want["shape"] == 2
    assert medium_report(f"{name} kind {kind} {set_name}, ending inside a medium", got["t"][fog], want["t"][fog]) <= MEDIUM_REL
    assert np.all(got["uv"][fog] == 0) and np.all(got["normal"][fog] == 0), "a medium hit has no surface (include/rtow.h rt_query_hits)"
    print(f"{name} kind {kind} {set_name}: {hit.sum()} hits of {len(o)}: {ball.sum()} on spheres (worst uv difference {err.max(initial=0):.3g}), "
          f"{flat.sum()} on quads and box faces, {fog.sum()} inside media")


@pytest.mark.parametrize("set_name", RW.SETS)
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_occlusion_is_the_references_hit_flag(name, kind, set_name):
    fx, scene = fixture(), scene_of(name, kind)
    o, d, time, tmin, tmax = fx.rays(name, set_name)
    want = fx.hits(name, kind, set_name)["hit"] != 0
    got = scene.occluded(o, d, times=time, tmin=tmin, tmax=tmax, seed=RW.SEED, variant=0)
    flips = np.flatnonzero(got != want)
    assert len(flips) == 0, f"{len(flips)} decisions differ; the reference {'hits' if want[flips[0]] else 'misses'}: " + describe(flips[0], o, d, time, tmin, tmax)


@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_the_fast_build_agrees_on_the_free_rays_where_it_reports_the_same_leaf(name, kind):
    """As tests/test_ray_query_gpu.py test_strict_and_fast_agree_where_they_report_the_same_leaf: contraction may decide a comparison
    the other way, so where the two builds name the same leaf t agrees to 1e-12 relative; how often they name another is printed."""
    fx, scene = fixture(), scene_of(name, kind)
    o, d, time, tmin, tmax = fx.rays(name, "free")
    strict, fast = (scene.intersect(o, d, times=time, tmin=tmin, tmax=tmax, seed=RW.SEED, variant=v, want=("t", "leaf")) for v in (0, 1))
    same = strict["leaf"] == fast["leaf"]
    hit = same & (strict["leaf"] >= 0)
    rel = np.abs(strict["t"][hit] - fast["t"][hit]) / strict["t"][hit]
    print(f"{name} kind {kind}: the leaf differs on {np.sum(~same)} of {same.size} rays; same leaf: worst relative t difference {rel.max():.3g}")
    assert hit.sum() > 50 and rel.max() <= 1e-12


# ---- Scene.path_step ----
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_one_bounce_is_the_references(name, kind):
    fx, scene = fixture(), scene_of(name, kind)
    o, d, time = fx.step_rays(name)
    streams = fx.streams()
    want = fx.steps(name, kind)
    got = scene.path_step(o, d, times=time, rng_state=streams, variant=0,
                          want=("status", "emitted", "attenuation", "origin", "direction", "time", "t", "front_face", "material", "rng_state"))

    def first_wrong(key, rows, positive_zero=False):
        w = want[key] + 0.0 if positive_zero else want[key]   # (the step gives a negative zero back as a positive one, include/rtow.h)
        wrong = np.flatnonzero(rows & np.any((bits(got[key]) != bits(w)).reshape(len(o), -1), axis=-1))
        assert len(wrong) == 0, f"{key}: {got[key][wrong[0]]!r} != {w[wrong[0]]!r} ({len(wrong)} rays), ray {wrong[0]}: origin {o[wrong[0]].tolist()} " \
                                f"direction {d[wrong[0]].tolist()} time {time[wrong[0]]!r} stream {streams[wrong[0]].tolist()}"

    everyone = np.ones(len(o), dtype=bool)
    for key in ("status", "rng_state", "material", "front_face", "time"):   # decisions and draws: exact for every ray
        first_wrong(key, everyone)
    fog, marble = want["flags"] & 1 != 0, want["flags"] & 2 != 0
    for key in ("t", "origin", "direction"):
        first_wrong(key, ~fog)
    first_wrong("direction", fog)   # an isotropic direction comes from the stream alone, a surface behind a medium from the surface
    first_wrong("emitted", everyone, positive_zero=True)       # no light of these worlds has a noise texture
    first_wrong("attenuation", ~marble, positive_zero=True)    # a medium's colour, a surface's behind it: nothing of t in them
    err = np.abs(got["attenuation"][marble] - want["attenuation"][marble])
    assert np.all(err <= NOISE_ABS)
    # rays whose search drew in a medium: t within the medium's bound, the origin what such a t makes of o + t * d -- the
    # difference of t through the product, and the roundings of the product and of the sum, half an ulp each on either side
    ended = fog & (want["status"] != 0)
    assert medium_report(f"{name} kind {kind} steps, hits after a draw in a medium", got["t"][ended], want["t"][ended]) <= MEDIUM_REL
    moved = fog & (want["status"] == 2)
    reach = np.abs(want["t"][moved, None] * d[moved])
    bound = MEDIUM_REL * reach + 2.0 ** -52 * (reach + np.abs(want["origin"][moved]))
    err_o = np.abs(got["origin"][moved] - want["origin"][moved])
    assert np.all(err_o <= bound)
    first_wrong("origin", fog & (want["status"] != 2))   # the ray that came in
    print(f"{name} kind {kind} steps: status {np.bincount(want['status'], minlength=3).tolist()}, {fog.sum()} met a medium (origins bit-exact: "
          f"{float(np.mean(np.all(bits(got['origin'][moved]) == bits(want['origin'][moved]), axis=-1))) if moved.any() else 1.0:.4f}), "
          f"{marble.sum()} a noise texture (worst colour difference {err.max(initial=0):.3g}, bound {NOISE_ABS:.3g})")


# ---- whole paths ----
@pytest.mark.parametrize("name, kind", CASES, ids=IDS)
def test_whole_paths_are_the_fold_of_the_references_steps(name, kind):
    """Scene.radiance(samples=1) and PathBatch.run of the inside rays against the reference's steps folded by the generator: bit for
    bit on the paths that met no medium and no noise texture; the chain of equalities of the camera rays, once off the camera."""
    fx, scene = fixture(), scene_of(name, kind)
    o, d, time = (np.ascontiguousarray(a[512:]) for a in fx.step_rays(name))
    streams = np.ascontiguousarray(fx.streams()[512:])
    want, exact = fx.of(name, "radiance", kind), fx.of(name, "radiance_exact", kind)
    assert exact.sum() >= 64
    got = scene.radiance(o, d, times=time, samples=1, max_depth=50, rng_state=streams, variant=0)["radiance"]
    differ = np.flatnonzero(exact & np.any(bits(got) != bits(want), axis=-1))
    assert len(differ) == 0, f"{len(differ)} paths differ, the first: ray {differ[0]} {got[differ[0]]!r} != {want[differ[0]]!r}"
    batch = rt.PathBatch(scene, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), times=torch.from_numpy(time).cuda(),
                         rng_state=torch.from_numpy(streams.view(np.int32)).cuda(), variant=0)
    ran = batch.run(50).cpu().numpy()
    assert np.array_equal(bits(ran[exact]), bits(want[exact]))
    rest = np.abs(got[~exact] - want[~exact])
    print(f"{name} kind {kind}: {exact.sum()} of {len(o)} paths bit for bit; the other {np.sum(~exact)} met a medium or a noise texture: "
          f"{float(np.mean(np.all(bits(got[~exact]) == bits(want[~exact]), axis=-1))) if rest.size else 1.0:.4f} of them bit-exact too, "
          f"worst difference {rest.max(initial=0):.3g}")
