"""The environment on the device: the value of a miss against the numpy restatement (tests/environment_restated.py) through
``path_step``, the twin scene that pins the mapping to the reference's GetSphereUV, one environment through every route that ends
in a miss, the importance sampler against its restatement and its tables, and what the sampler is for.  Every ray set is a few
hundred to a few thousand rays, every frame 16 x 16; the sampler's counts take 65 536 points."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import environment_restated as E
import film_direct_restated as fdr
import raytracinginoneweekendincuda_amd as rt
from conftest import ROOT
from light_restated import PI, seeded_states
from query_helpers import bits, centre_rays
from test_path_step_gpu import fold
from triangle_meshes import icosphere

pytestmark = pytest.mark.gpu

SEED = 1984
W = H = 16
SPP, DEPTH = 4, 8
MISS, ENDS, SCATTERED = 0, 1, 2
TILT = E.rotation((1.0, 2.0, 3.0), 40.0)        # not axis-aligned
TINT = (0.25, 3.0, 1.5)


def float_map(w, h, seed=11):
    return np.random.default_rng(seed).uniform(0.05, 2.0, size=(h, w, 3)).astype(np.float32)


def byte_map(w, h, seed=12):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def random_directions(n, seed=5):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return np.ascontiguousarray(d * np.random.default_rng(seed + 1).uniform(0.2, 7.0, size=(n, 1)))   # not unit


def open_scene(environment, lamp_texture=None):
    """Nothing to hit from the origin but a speck far away; a black background.  ``environment(s)``: the arguments of
    Scene.Environment.  ``lamp_texture(s)``: instead, the twin -- a unit DiffuseLight sphere of that texture about the origin."""
    s = rt.Scene()
    speck = s.Sphere((1000.0, 1000.0, 1000.0), 1e-3, s.Lambertian((0.5, 0.5, 0.5)))
    if lamp_texture is not None:
        s.SetWorld(s.HittableList([speck, s.Sphere((0, 0, 0), 1.0, s.DiffuseLight(lamp_texture(s)))]))
    else:
        s.SetWorld(s.HittableList([speck]))
        s.Environment(**environment(s))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60.0, 1.0, 0.0, 1.0, background=(0, 0, 0))
    s.Commit()
    return s


def emitted_along(scene, d, status=MISS, variant=0):
    out = scene.path_step(np.zeros_like(d), np.ascontiguousarray(d), variant=variant, want=("status", "emitted"))
    assert np.all(out["status"] == status)
    return out["emitted"]


PLACEMENTS = [dict(), dict(intensity=TINT, rotation=TILT)]


def placed(kw):
    return np.asarray(kw.get("intensity", (1.0, 1.0, 1.0)), dtype=np.float64), kw.get("rotation", np.eye(3))


# ---- 1. the value, bit for bit ----
@pytest.mark.parametrize("kw", PLACEMENTS)
def test_a_solid_environment(kw):
    k, R = placed(kw)
    got = emitted_along(open_scene(lambda s: dict(texture=s.SolidColor((0.3, 0.6, 0.9)), **kw)), random_directions(500))
    assert np.array_equal(bits(got), bits(np.broadcast_to(k * np.array((0.3, 0.6, 0.9)), got.shape)))


@pytest.mark.parametrize("kw", PLACEMENTS)
def test_a_checker_environment_is_a_function_of_the_direction(kw):
    """The checker's input is e = R n, whose arithmetic is IEEE on both sides: no libm between the direction and the colour."""
    k, R = placed(kw)
    even, odd = (0.9, 0.8, 0.1), (0.05, 0.2, 0.4)
    scene = open_scene(lambda s: dict(texture=s.CheckerTexture(0.23, s.SolidColor(even), s.SolidColor(odd)), **kw))
    d = random_directions(2000)
    e, _, _ = E.coords(d, R)
    want = E.checker_value(1.0 / 0.23, even, odd, k, e)
    assert len(np.unique(want[:, 0])) == 2
    assert np.array_equal(bits(emitted_along(scene, d)), bits(want))


@pytest.mark.parametrize("kw", PLACEMENTS)
@pytest.mark.parametrize("kind", ["8-bit", "float"])
def test_image_environments_through_texel_centres(kind, kw):
    k, R = placed(kw)
    for w, h in ((8, 4), (3, 2), (1, 1), (37, 19)):
        img = byte_map(w, h) if kind == "8-bit" else float_map(w, h)
        scene = open_scene(lambda s: dict(texture=s.ImageTexture(img), **kw) if kind == "8-bit" else dict(image=img, **kw))
        d = E.centre_directions(w, h, R, length=2.5)
        _, u, v = E.coords(d, R)
        i, j = E.texel(w, h, u, v)
        assert np.array_equal(j * w + i, np.arange(w * h)), "every texel is looked up once, in order"
        assert np.array_equal(bits(emitted_along(scene, d)), bits(E.image_value(img, k, u, v)))


@pytest.mark.parametrize("w,h", [(8, 4), (3, 2)])
def test_image_environments_along_random_directions(w, h):
    """acos and atan2 are each library's own: the rays whose restated (u, v), moved by +-4 ulp, name another texel are left out
    -- at most 1 % of them, checked here on the CPU for the seed used -- and every other ray agrees bit for bit."""
    img = float_map(w, h)
    d = random_directions(4000, seed=21)
    _, u, v = E.coords(d, TILT)
    keep = E.texel_is_stable(w, h, u, v)
    assert keep.mean() >= 0.99
    got = emitted_along(open_scene(lambda s: dict(image=img, intensity=TINT, rotation=TILT)), d)
    want = E.image_value(img, TINT, u, v)
    assert np.array_equal(bits(got[keep]), bits(want[keep]))
    assert len(np.unique(E.texel(w, h, u, v)[0] + w * E.texel(w, h, u, v)[1])) == w * h, "every texel is reached"


# ---- 2. the twin: the reference's own sphere mapping ----
def quadruple_directions():
    """Integer directions whose length is an integer k: then 1 / sqrt(d.d) and the sphere's root sqrt(d.d) / d.d are both fl(1 / k),
    the environment's n and the twin's hit point are the same bits, and so is whatever a texture makes of them."""
    r = np.arange(-9, 10)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(r, r, r, indexing="ij"))
    n2 = x * x + y * y + z * z
    k = np.rint(np.sqrt(n2)).astype(np.int64)
    pick = (k * k == n2) & (n2 > 0) & ((x != 0) | (z != 0))
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1)[pick].astype(np.float64))


def relative_error(a, b):
    scale = np.maximum(np.abs(a), np.abs(b))
    return np.max(np.where(scale > 0.0, np.abs(a - b) / np.where(scale > 0.0, scale, 1.0), 0.0))


@pytest.mark.parametrize("name", ["solid", "noise", "image"])
def test_the_twin_scene_with_an_emissive_unit_sphere_emits_the_same(name):
    """Scene B is scene A without its environment and with a unit DiffuseLight(T) sphere about the origin: the reference's own
    GetSphereUV orientation, not a convention of this library's."""
    img = byte_map(8, 4)
    texture = {"solid": lambda s: s.SolidColor((0.2, 0.7, 1.3)), "noise": lambda s: s.NoiseTexture(4.0, rt.Rng(SEED, 0)),
               "image": lambda s: s.ImageTexture(img)}[name]
    d = {"solid": random_directions(500), "noise": quadruple_directions(), "image": E.centre_directions(8, 4, length=3.0)}[name]
    assert len(d) >= 32
    a = emitted_along(open_scene(lambda s: dict(texture=texture(s))), d)
    b = emitted_along(open_scene(None, lamp_texture=texture), d, status=ENDS)
    worst = relative_error(a, b)
    print(f"twin {name}: {len(d)} rays, largest relative difference {worst:.3g}")
    assert worst <= 1e-12
    assert len(np.unique(a, axis=0)) >= (1 if name == "solid" else 8)


def test_a_noise_environment_along_random_directions():
    """The tolerance tests/test_shading_gpu.py grants NoiseTexture on the device (at least 99.9 % within 1e-5: device sin differs
    from any other by an ulp, and the marble amplifies the last bits of the point), against the twin's emissive sphere."""
    texture = lambda s: s.NoiseTexture(4.0, rt.Rng(SEED, 0))
    d = random_directions(2000, seed=31)
    a = emitted_along(open_scene(lambda s: dict(texture=texture(s))), d)
    b = emitted_along(open_scene(None, lamp_texture=texture), d, status=ENDS)
    within = np.mean(np.all(np.abs(a - b) <= 1e-5, axis=-1))
    print(f"noise environment against its twin: within 1e-5 {within:.4f}, bit-equal {np.mean(np.all(bits(a) == bits(b), axis=-1)):.4f}")
    assert within >= 0.999 and a.std() > 0.05


# ---- 3. one environment, every route ----
SKY = dict(image=float_map(8, 4, seed=41), intensity=(1.0, 0.8, 1.2), rotation=TILT)


def route_world(name):
    s = rt.Scene()
    grey, metal, glass = s.Lambertian((0.6, 0.55, 0.5)), s.Metal((0.8, 0.8, 0.7), 0.1), s.Dielectric(1.5)
    ground = s.Sphere((0, -100.5, 0), 100.0, s.Lambertian((0.4, 0.5, 0.3)))
    few = [ground, s.Sphere((0, 0, 0), 0.5, grey), s.Sphere((1.1, 0, 0.2), 0.5, metal), s.Sphere((-1.1, 0, 0.3), 0.5, glass),
           s.Translate(s.MakeBox((-0.3, 0, -0.3), (0.3, 0.6, 0.3), grey), (0.2, -0.5, 1.2))]
    if name == "list":
        world = s.HittableList(few)
    elif name == "bvh":
        world = s.BvhNode(few)
    elif name == "deep bvh":     # more than 64 nodes: the deep instantiation
        rng = np.random.default_rng(3)
        world = s.BvhNode([ground] + [s.Sphere((x, -0.3, z), 0.18, (grey, metal, glass)[k % 3])
                                      for k, (x, z) in enumerate(rng.uniform(-2.5, 2.5, size=(90, 2)))])
    elif name == "moving mesh":  # a MovingTransform over a mesh: the second pass of the affine units
        v, f = icosphere(1, 0.6)
        mesh = s.TriangleMesh(v, f, grey)
        m0 = np.hstack([np.eye(3), [[-0.6], [0.1], [0.0]]])
        m1 = np.hstack([1.2 * np.eye(3), [[0.6], [0.3], [0.0]]])
        world = s.HittableList([ground, s.MovingTransform(mesh, m0, m1, 0.0, 1.0), s.Sphere((0, 0, -1.5), 0.5, metal)])
    else:                        # "lamp": the list world and a lamp, for the routes with light samples
        world = s.HittableList(few + [s.Quad((-1, 2.0, -1), (2, 0, 0), (0, 0, 2), s.DiffuseLight((6.0, 5.0, 4.0)))])
    s.SetWorld(world)
    s.Camera((0.5, 1.2, 4.5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.05, 4.5, 0.0, 1.0, background=(0, 0, 0))
    s.Environment(**SKY)
    s.Commit()
    return s


@functools.lru_cache(maxsize=None)
def routes_of(name, variant=0):
    scene = route_world(name)
    film = rt.Film(W, H)
    st = film.render(scene, SPP, max_depth=DEPTH, seed=SEED, variant=variant)
    return scene, film.download(), st


def to_device(a):
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("name", ["list", "bvh", "deep bvh", "moving mesh"])
def test_every_route_sees_the_same_environment(name):
    scene, frame, st = routes_of(name)
    print(f"{name}: kernel kind {st.kernel_kind}, lds {st.lds_bytes}, {st.rays} rays, mean {frame.mean():.4f}")
    assert st.kernel_kind & 1, "a rich instantiation"
    if name == "deep bvh":
        # kind 7 is the general and the deep instantiation alike; the plan of this very launch names the kernel (launch_plan.h KernelId)
        plan = scene.plan_launch(rt.Film(W, H).params(SPP, max_depth=DEPTH, seed=SEED, variant=0))
        assert st.kernel_kind == 7 and scene.info()["n_nodes"] > 64 and plan["kernel"] == 13, "K_BVH_GENERAL_DEEP"
    assert frame.mean() > 0.05, "the background is black: all the light is the environment's"
    # the adaptive frame, at a rule that stops nothing before the cap
    film = rt.Film(W, H)
    film.set_adaptive(SPP, 1, 0.0)
    ast = film.render(scene, SPP, max_depth=DEPTH, seed=SEED, variant=0)
    assert ast.kernel_kind & 512 and np.all(film.sample_counts() == SPP)
    assert np.array_equal(bits(film.download()), bits(frame))
    # the frame restated through Scene.radiance fed the frame's camera rays and streams, sample by sample
    plain = fdr.Frame(scene, W, H, SEED).launch(SPP, DEPTH, direct=False)
    assert np.array_equal(bits(plain.pixels()), bits(frame)) and plain.rays == st.rays and plain.longest_path > 1
    # the first sample's rays: the radiance query, the host fold of path steps, and PathBatch.run
    o, d, tm, states = fdr.camera_rays_from(scene, fdr.seeded_states(SEED, W, H), W, H)
    rad = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, variant=0, want=("radiance", "path_rays", "rng_state"))
    seen = {"status": set(), "material": set()}
    acc, steps, final = fold(scene, o, d, tm, states, DEPTH, seen)
    assert MISS in seen["status"], "paths end in the environment"
    assert np.array_equal(bits(acc), bits(rad["radiance"])) and np.array_equal(steps, rad["path_rays"]) and np.array_equal(final, rad["rng_state"])
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states))
    run = batch.run(DEPTH)
    torch.cuda.synchronize()
    assert np.array_equal(bits(run.cpu().numpy()), bits(rad["radiance"]))
    # no lamps in this world: the three routes with light samples are the plain routes
    assert scene.info()["n_lights"] == 0
    direct = rt.Film(W, H)
    dst = direct.render(scene, SPP, direct="mis", max_depth=DEPTH, seed=SEED, variant=0)
    assert dst.kernel_kind & 1024 and np.array_equal(bits(direct.download()), bits(frame))
    mis = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, variant=0, direct="mis")["radiance"]
    assert np.array_equal(bits(mis), bits(rad["radiance"]))
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), direct="mis")
    run = batch.run(DEPTH)
    torch.cuda.synchronize()
    assert np.array_equal(bits(run.cpu().numpy()), bits(rad["radiance"]))


def test_the_routes_with_light_samples_agree_under_an_environment():
    scene = route_world("lamp")
    assert scene.info()["n_lights"] == 1
    film = rt.Film(W, H)
    st = film.render(scene, SPP, direct="mis", max_depth=DEPTH, seed=SEED, variant=0)
    want = fdr.Frame(scene, W, H, SEED).launch(SPP, DEPTH, direct=True)      # Scene.radiance(direct="mis"), sample by sample
    assert np.array_equal(bits(film.download()), bits(want.pixels())) and want.shadow_rays > 0
    o, d, tm, states = fdr.camera_rays_from(scene, fdr.seeded_states(SEED, W, H), W, H)
    mis = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, variant=0, direct="mis")["radiance"]
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), direct="mis")
    run = batch.run(DEPTH)
    torch.cuda.synchronize()
    assert np.array_equal(bits(run.cpu().numpy()), bits(mis))
    plain = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, variant=0)["radiance"]
    assert not np.array_equal(bits(plain), bits(mis)), "the light samples do something here"


@pytest.mark.parametrize("name", ["list", "bvh"])
def test_the_feature_pass_records_the_environment_as_the_albedo_of_a_miss(name):
    scene, _, _ = routes_of(name)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0)
    albedo, normal, depth = (a.reshape(W * H, -1) for a in film.features())
    o, d, tm, _ = centre_rays(scene, W, H)
    hit = scene.intersect(o, d, time=tm, want=("t", "albedo"))
    miss = np.isinf(hit["t"])
    assert 10 < miss.sum() < W * H - 10
    _, u, v = E.coords(d, SKY["rotation"])
    keep = miss & E.texel_is_stable(8, 4, u, v)
    assert keep.sum() >= 0.9 * miss.sum()
    want = 0.0 + E.image_value(SKY["image"], SKY["intensity"], u, v)
    assert np.array_equal(bits(albedo[keep]), bits(want[keep])) and np.array_equal(bits(hit["albedo"][keep]), bits(want[keep]))
    assert not normal[miss].any() and not depth[miss].any()


# ---- 4. the sampler ----
def sun_map():
    img = float_map(8, 4, seed=51)
    img[1, 5] = 1000.0 * img[1, 5]       # one texel 1000 times the others
    return img


def zero_row_map():
    img = float_map(3, 2, seed=52)
    img[1] = 0.0
    return img


SAMPLER_MAPS = {"sun 8x4": sun_map, "zero row 3x2": zero_row_map, "1x1": lambda: float_map(1, 1, seed=53)}
N_BITS = 4096


@functools.lru_cache(maxsize=None)
def host_states():
    s = seeded_states(N_BITS, SEED)
    s.setflags(write=False)
    return s


def sampler_scene(img, **kw):
    return open_scene(lambda s: dict(image=img, **kw))


def check_against_restatement(scene, img, intensity, R, n=N_BITS):
    """The draws, the direction, the density and the value of n samples against the restatement and against the other calls."""
    h, w = img.shape[:2]
    cdf = scene.environment_cdf()
    want_cdf = E.build_cdf(img, intensity)
    assert (cdf is None) == (want_cdf is None)
    states = np.array(host_states()[:n])
    points = np.zeros((n, 3))
    got = scene.sample_environment(points, rng_state=states)
    want = E.sample(cdf, w, h, states, R)
    assert want["valid"].mean() >= 0.999, "the restatement, on the CPU, for the seed used"
    valid = got["pdf"] > 0.0
    assert valid.mean() >= 0.999
    assert np.array_equal(got["light"], want["texel"]), "the texel the draws pick"
    assert np.array_equal(got["rng_state"], want["rng_state"]), "four draws"
    both = valid & want["valid"]
    assert np.max(np.abs(got["direction"][both] - want["direction"][both])) <= 1e-12
    assert np.all(np.isinf(got["distance"][valid])) and not got["distance"][~valid].any() and not got["direction"][~valid].any()
    # the density of the final direction: the texel the device's own lookup names, the tables' factor and the Jacobian restated
    d = np.ascontiguousarray(got["direction"][valid])
    looked = scene.environment_pdf(np.zeros_like(d), d, want=("pdf", "light"))
    assert np.array_equal(bits(looked["pdf"]), bits(got["pdf"][valid])), "environment_pdf(direction) is the sampled pdf"
    e, _, _ = E.coords(d, R)
    if cdf is not None:
        j, i = np.divmod(looked["light"].astype(np.int64), w)
        pj = cdf[0][j] - np.where(j > 0, cdf[0][np.maximum(j - 1, 0)], 0.0)
        pi = cdf[1][j, i] - np.where(i > 0, cdf[1][j, np.maximum(i - 1, 0)], 0.0)
        pdf = ((pj * pi) * (float(w) * float(h))) / (((2.0 * PI) * PI) * np.sqrt(1.0 - e[:, 1] * e[:, 1]))
        assert np.array_equal(bits(pdf), bits(got["pdf"][valid])), "the tables' factor and the Jacobian"
        assert np.mean(looked["light"] == got["light"][valid]) >= 0.999, "the direction lies in the texel drawn"
    else:
        assert np.all(looked["light"] == -1) and np.array_equal(bits(got["pdf"][valid]), bits(np.full(valid.sum(), 1.0 / (4.0 * PI))))
    # the value: the lookup of the direction, through a path step
    assert np.array_equal(bits(emitted_along(scene, d)), bits(got["emitted"][valid]))
    return got, cdf


@pytest.mark.parametrize("kw", PLACEMENTS)
@pytest.mark.parametrize("name", sorted(SAMPLER_MAPS))
def test_samples_equal_the_restatement(name, kw):
    img = SAMPLER_MAPS[name]()
    k, R = placed(kw)
    got, cdf = check_against_restatement(sampler_scene(img, **kw), img, k, R)
    if name == "zero row 3x2":
        assert np.all(got["light"] < 3), "zero-weight texels are never drawn"
    if name == "1x1":
        assert np.all(got["light"] == 0) and np.all(got["pdf"] > 0.0)


def test_the_uniform_fallback_for_a_checker_sky():
    scene = open_scene(lambda s: dict(texture=s.CheckerTexture(0.4, s.SolidColor((1, 1, 1)), s.SolidColor((0.1, 0.1, 0.1))), rotation=TILT))
    assert not scene.environment()["has_distribution"]
    states = np.array(host_states())
    got = scene.sample_environment(np.zeros((N_BITS, 3)), rng_state=states)
    want = E.sample(None, 0, 0, states, TILT)
    assert np.all(got["light"] == -1) and np.array_equal(bits(got["pdf"]), bits(np.full(N_BITS, 1.0 / (4.0 * PI))))
    assert np.max(np.abs(got["direction"] - want["direction"])) <= 1e-12 and np.array_equal(got["rng_state"], want["rng_state"])
    assert np.array_equal(bits(emitted_along(scene, got["direction"])), bits(got["emitted"]))
    assert np.max(np.abs(got["direction"].mean(axis=0))) < 5.0 / np.sqrt(3.0 * N_BITS), "uniform over the sphere: mean 0, variance 1/3 a coordinate"


@pytest.mark.parametrize("rows", [0, 1])
def test_both_sides_of_the_cap_of_the_staged_marginal_table(rows):
    h = rt._lib.env_lds_rows() + rows
    img = float_map(2, h, seed=61)
    img[-1] *= 1e6            # the last row -- the one beyond the cap where there is one -- is drawn often, although it lies at a pole
    img[h // 2] *= 300.0
    got, cdf = check_against_restatement(sampler_scene(img), img, np.ones(3), np.eye(3))
    rows_drawn = got["light"] // 2
    assert np.sum(rows_drawn == h - 1) > 100 and np.sum(rows_drawn == h // 2) > 100 and len(np.unique(rows_drawn)) > 500


@pytest.mark.parametrize("name", ["sun 8x4", "zero row 3x2"])
def test_counts_and_the_estimate_of_the_integral_over_65536_samples(name):
    img = SAMPLER_MAPS[name]()
    h, w = img.shape[:2]
    scene = sampler_scene(img, intensity=TINT, rotation=TILT)
    n = 65536
    got = scene.sample_environment(np.zeros((n, 3)), seed=SEED + 1, want=("light", "pdf", "emitted"))
    marginal, conditional = scene.environment_cdf()
    P = (np.diff(marginal, prepend=0.0)[:, None] * np.diff(conditional, axis=1, prepend=0.0)).reshape(-1)
    P[np.repeat(np.diff(marginal, prepend=0.0) == 0.0, w)] = 0.0
    counts = np.bincount(got["light"], minlength=w * h)
    sigma = np.sqrt(n * P * (1.0 - P))
    assert np.all(np.abs(counts - n * P) <= 5.0 * sigma), "every texel within 5 binomial standard deviations"
    assert np.all(counts[P == 0.0] == 0), "zero-weight texels are never drawn"
    valid = got["pdf"] > 0.0
    assert valid.mean() >= 0.999
    ratio = np.where(valid[:, None], got["emitted"] / np.where(valid, got["pdf"], 1.0)[:, None], 0.0)
    mean, err = ratio.mean(axis=0), ratio.std(axis=0, ddof=1) / np.sqrt(n)
    exact = E.integral(img, TINT)
    print(f"{name}: mean(emitted / pdf) {mean}, exact {exact}, standard errors {err}")
    assert np.all(np.abs(mean - exact) <= 5.0 * err)


# ---- 5. the executable ----
@pytest.mark.parametrize("case", ["scene 15", "--environment"])
def test_rtow_traces_the_environment_the_api_traces(case, tmp_path):
    """rtow --scene 15, and rtow --environment FILE.pfm --environment-intensity X --environment-rotate-y DEG over a scene that has
    none: --radiance-at prints what Scene.radiance returns for the same scene built through the API."""
    i, j, spp = 3, 13, 2
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    if case == "scene 15":
        options, scene = ["--scene", "15"], rt.sky_demo_scene(0, W, H)
        assert scene.flags() & rt.SCENE_FLAG_ENVIRONMENT and scene.environment()["has_distribution"]
    else:
        sky = float_map(8, 4, seed=71)
        rt.write_pfm(tmp_path / "sky.pfm", sky[::-1].astype(np.float64))       # a frame's rows are bottom first
        options = ["--scene", "10", "--environment", str(tmp_path / "sky.pfm"), "--environment-intensity", "2.5", "--environment-rotate-y", "30"]
        scene = rt.builtin_scene(10, 0, W, H)
        cs, sn = math.cos(30.0 * PI / 180.0), math.sin(30.0 * PI / 180.0)
        scene.Environment(image=rt.load_pfm(tmp_path / "sky.pfm"), intensity=2.5, rotation=[[cs, 0.0, -sn], [0.0, 1.0, 0.0], [sn, 0.0, cs]])
        scene.Commit()
        assert np.array_equal(bits(scene.environment()["image"]), bits(sky))
    run = subprocess.run([exe, *options, "--width", str(W), "--height", str(H), "--variant", "strict", "--spp", str(spp), "--radiance-at", f"{i},{j}"],
                         check=True, cwd=ROOT, timeout=120, capture_output=True, text=True)
    words = [line for line in run.stdout.splitlines() if line.startswith("radiance ")][0].split()
    o, d, time0, _ = centre_rays(scene, W, H)
    k = j * W + i
    out = scene.radiance(o[k:k + 1].copy(), d[k:k + 1].copy(), time=time0, samples=spp, first_sequence=k, want=("radiance", "path_rays"))
    assert [float(x) for x in words[5:8]] == list(out["radiance"][0]) and any(out["radiance"][0])
    assert int(words[9]) == out["path_rays"][0]


# ---- 6. what the sampler is for ----
def test_sampling_the_sun_beats_finding_it_by_scattering():
    """A Lambertian ground and an occluding box under scene 15's sky reduced to 64 x 32: at 512 points of the ground, next-event
    estimation with sample_environment (B) agrees with Scene.radiance (A) and has the smaller standard error."""
    sky = rt.sky_demo_scene(1, 16, 16).environment()["image"]
    assert sky.shape == (128, 256, 3) and sky.max() > 1000.0
    small = sky.reshape(32, 4, 64, 4, 3).mean(axis=(1, 3)).astype(np.float32)
    s = rt.Scene()
    ground = s.Quad((-20, 0, -20), (40, 0, 0), (0, 0, 40), s.Lambertian((0.7, 0.7, 0.7)))
    s.SetWorld(s.HittableList([ground, s.MakeBox((-1, 0, -1), (1, 2, 1), s.Lambertian((0.3, 0.3, 0.3)))]))
    s.Camera((0, 5, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, background=(0, 0, 0))
    s.Environment(image=small)
    s.Commit()
    n, samples = 512, 64
    rng = np.random.default_rng(7)
    target = np.stack([rng.uniform(-6, 6, 2 * n), np.zeros(2 * n), rng.uniform(-6, 6, 2 * n)], axis=-1)
    target = target[(np.abs(target[:, 0]) > 1.2) | (np.abs(target[:, 2]) > 1.2)][:n]
    assert len(target) == n
    o = np.ascontiguousarray(target + np.array((0.0, 6.0, 0.0)))     # straight down onto the ground, beside the box
    d = np.ascontiguousarray(np.broadcast_to((0.0, -1.0, 0.0), (n, 3)))
    # A: whole paths of two bounces; the second ray finds the sky, or not
    a = np.stack([s.radiance(o, d, samples=1, max_depth=2, first_sequence=k * n)["radiance"] for k in range(samples)])
    # B: the first bounce's hit, a sample of the environment there, its shadow ray
    b = []
    for k in range(samples):
        hit = s.path_step(o, d, first_sequence=k * n, want=("status", "attenuation", "origin", "normal", "material", "rng_state"))
        assert np.all(hit["status"] == SCATTERED)
        smp = s.sample_environment(hit["origin"], normals=hit["normal"], materials=hit["material"], rng_state=hit["rng_state"],
                                   want=("direction", "distance", "contribution"))
        args = s.shadow_rays(hit["origin"], smp["direction"], smp["distance"])
        assert np.all(np.isinf(args[4][smp["distance"] > 0.0])), "tmax = inf"
        lit = ~s.occluded(*args) & (smp["distance"] > 0.0)
        b.append(np.where(lit[:, None], hit["attenuation"] * smp["contribution"], 0.0))
    b = np.stack(b)
    lum = lambda x: x.sum(axis=-1).mean(axis=1)            # per batch: the mean over the points of r + g + b
    ma, mb = lum(a).mean(), lum(b).mean()
    ea, eb = lum(a).std(ddof=1) / np.sqrt(samples), lum(b).std(ddof=1) / np.sqrt(samples)
    print(f"sun: A (radiance) {ma:.5f} +- {ea:.5f}, B (sample_environment) {mb:.5f} +- {eb:.5f}, ratio of standard errors {ea / eb:.2f}")
    assert abs(ma - mb) <= 5.0 * np.hypot(ea, eb)
    assert eb < ea
