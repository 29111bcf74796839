"""The environment in the fast build (variant=1, -ffp-contract=fast): the value of a miss through ``path_step``, one environment
through every route that ends in a miss, and the importance sampler -- a kernel of its own in this build -- against the
restatement (tests/environment_restated.py), its tables and the density call.  The strict build is pinned bit for bit by
tests/test_environment_gpu.py, whose scenes, maps and directions these are.  Where a lookup may fall on either side of a texel's
or a checker's edge under contraction the ray is left out by a margin computed from the restatement on the CPU, whose share is
asserted there; values are held to bounds from conditioning, and the measured worst is printed.  Every ray set is 500 to 4096
directions, every frame 16 x 16; the sampler's counts take 65 536 points."""

import numpy as np
import pytest

import environment_restated as E
import film_direct_restated as fdr
import raytracinginoneweekendincuda_amd as rt
import test_environment_gpu as eg
from light_restated import PI
from query_helpers import bits, uv_bound
from test_environment_gpu import ENDS, PLACEMENTS, SAMPLER_MAPS, SEED, SKY, TILT, TINT, W, H, DEPTH
from test_environment_gpu import byte_map, emitted_along, float_map, open_scene, placed, random_directions, relative_error, sampler_scene
from test_fast_instances_gpu import check_routes_and_frames

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


# ---- the margins, from the restatement alone (CPU) ----
def texel_is_far_from_an_edge(w, h, e, u, v):
    """(u, v) are functions of e = R n (query_helpers.uv_bound has the conditioning; e is good to far less than its 1e-12 in
    either build): is the restated (u, v) further than that bound from every edge of the w x h grid, the seam and the poles
    included?"""
    bound = uv_bound(e)[:, 0]
    du = np.abs(u - np.rint(u * w) / w)
    dv = np.abs(v - np.rint(v * h) / h)
    with np.errstate(invalid="ignore"):
        return (du > bound) & (dv > bound)


def checker_is_stable(inv_scale, e):
    x = inv_scale * e
    return (np.abs(x - np.rint(x)) > 1e-12).all(axis=1)


# ---- 1. the value ----
@pytest.mark.parametrize("kw", PLACEMENTS)
def test_a_solid_environment_in_the_fast_build(kw):
    k, R = placed(kw)
    got = emitted_along(open_scene(lambda s: dict(texture=s.SolidColor((0.3, 0.6, 0.9)), **kw)), random_directions(500), variant=1)
    assert np.array_equal(bits(got), bits(np.broadcast_to(k * np.array((0.3, 0.6, 0.9)), got.shape))), "one multiply"


@pytest.mark.parametrize("kw", PLACEMENTS)
def test_a_checker_environment_in_the_fast_build(kw):
    k, R = placed(kw)
    even, odd = (0.9, 0.8, 0.1), (0.05, 0.2, 0.4)
    d = random_directions(2000)
    e, _, _ = E.coords(d, R)
    keep = checker_is_stable(1.0 / 0.23, e)
    assert keep.mean() >= 0.99
    want = E.checker_value(1.0 / 0.23, even, odd, k, e)
    scene = open_scene(lambda s: dict(texture=s.CheckerTexture(0.23, s.SolidColor(even), s.SolidColor(odd)), **kw))
    got = emitted_along(scene, d, variant=1)
    print(f"checker: {np.sum(~keep)} of {len(d)} rays left out")
    assert len(np.unique(want[keep, 0])) == 2 and np.array_equal(bits(got[keep]), bits(want[keep]))


@pytest.mark.parametrize("kw", PLACEMENTS)
@pytest.mark.parametrize("kind", ["8-bit", "float"])
def test_image_environments_through_texel_centres_in_the_fast_build(kind, kw):
    k, R = placed(kw)
    for w, h in ((8, 4), (3, 2), (1, 1), (37, 19)):
        img = byte_map(w, h) if kind == "8-bit" else float_map(w, h)
        scene = open_scene(lambda s: dict(texture=s.ImageTexture(img), **kw) if kind == "8-bit" else dict(image=img, **kw))
        d = E.centre_directions(w, h, R, length=2.5)
        _, u, v = E.coords(d, R)
        i, j = E.texel(w, h, u, v)
        assert np.array_equal(j * w + i, np.arange(w * h)), "every texel is looked up once, in order"
        assert np.array_equal(bits(emitted_along(scene, d, variant=1)), bits(E.image_value(img, k, u, v))), (w, h)


@pytest.mark.parametrize("w,h", [(8, 4), (3, 2)])
def test_image_environments_along_random_directions_in_the_fast_build(w, h):
    img = float_map(w, h)
    d = random_directions(4000, seed=21)
    e, u, v = E.coords(d, TILT)
    keep = texel_is_far_from_an_edge(w, h, e, u, v)
    assert keep.mean() >= 0.99
    got = emitted_along(open_scene(lambda s: dict(image=img, intensity=TINT, rotation=TILT)), d, variant=1)
    want = E.image_value(img, TINT, u, v)
    print(f"{w} x {h}: {np.sum(~keep)} of {len(d)} rays left out")
    assert np.array_equal(bits(got[keep]), bits(want[keep]))
    assert len(np.unique((E.texel(w, h, u, v)[0] + w * E.texel(w, h, u, v)[1])[keep])) == w * h, "every texel is reached"


@pytest.mark.parametrize("name", ["solid", "image"])
def test_the_twin_scene_in_the_fast_build(name):
    """tests/test_environment_gpu.py's twin: a unit DiffuseLight sphere of the texture about the origin, both in the fast build."""
    img = byte_map(8, 4)
    texture = {"solid": lambda s: s.SolidColor((0.2, 0.7, 1.3)), "image": lambda s: s.ImageTexture(img)}[name]
    d = {"solid": random_directions(500), "image": E.centre_directions(8, 4, length=3.0)}[name]
    a = emitted_along(open_scene(lambda s: dict(texture=texture(s))), d, variant=1)
    b = emitted_along(open_scene(None, lamp_texture=texture), d, status=ENDS, variant=1)
    worst = relative_error(a, b)
    print(f"twin {name}: {len(d)} rays, largest relative difference {worst:.3g}")
    assert worst <= 1e-12 and len(np.unique(a, axis=0)) >= (1 if name == "solid" else 8)


def test_a_noise_environment_along_random_directions_in_the_fast_build():
    texture = lambda s: s.NoiseTexture(4.0, rt.Rng(SEED, 0))
    d = random_directions(2000, seed=31)
    a = emitted_along(open_scene(lambda s: dict(texture=texture(s))), d, variant=1)
    b = emitted_along(open_scene(None, lamp_texture=texture), d, status=ENDS, variant=1)
    within = np.mean(np.all(np.abs(a - b) <= 1e-5, axis=-1))
    print(f"noise environment against its twin, both fast: within 1e-5 {within:.4f}, bit-equal {np.mean(np.all(bits(a) == bits(b), axis=-1)):.4f}")
    assert within >= 0.999 and a.std() > 0.05


# ---- 2. every route ----
@pytest.mark.parametrize("name", ["list", "bvh", "deep bvh", "moving mesh", "lamp"])
def test_every_route_sees_the_environment_in_the_fast_build(name):
    scene = eg.route_world(name)
    rays = fdr.camera_rays_from(scene, fdr.seeded_states(SEED, W, H), W, H)
    r = check_routes_and_frames(f"environment, {name}", scene, rays, W=W, H=H, depth=DEPTH)
    assert r["frame"].mean() > 0.05, "the background is black: all the light is the environment's (and the lamp's)"
    assert r["stats"].kernel_kind & 1, "a rich instantiation"
    # the albedo of a miss is the environment's value: the restated one, bit for bit, where the texel is named with a margin
    co, cd = r["centre_rays"]
    miss = np.isinf(r["seen"]["t"])
    e, u, v = E.coords(cd, SKY["rotation"])
    keep = miss & texel_is_far_from_an_edge(8, 4, e, u, v)
    assert miss.sum() > 10 and keep.sum() >= 0.99 * miss.sum()
    want = 0.0 + E.image_value(SKY["image"], SKY["intensity"], u, v)
    assert np.array_equal(bits(r["albedo"][keep]), bits(want[keep])) and np.array_equal(bits(r["seen"]["albedo"][keep]), bits(want[keep]))
    assert scene.info()["n_lights"] == (1 if name == "lamp" else 0)


# ---- 3. the sampler ----
N_BITS = eg.N_BITS


def check_sampler(label, scene, img, intensity, R, n=N_BITS):
    """``sample_environment(variant=1)`` against the restatement, the tables, ``environment_pdf`` and ``path_step``, all fast."""
    states = np.array(eg.host_states()[:n])
    points = np.zeros((n, 3))
    cdf = scene.environment_cdf()
    h, w = (img.shape[:2] if img is not None else (0, 0))
    want = E.sample(cdf, w, h, states, R)
    assert want["valid"].mean() >= 0.999, "the restatement, on the CPU, for the seed used"
    got, st = scene.sample_environment(points, rng_state=states, variant=1, stats=True)
    for key, a in got.items():
        if a.dtype == np.float64:
            assert not np.isnan(a).any(), key
    assert (got["pdf"] >= 0.0).all() and (got["emitted"] >= 0.0).all() and (got["distance"] >= 0.0).all()
    valid = got["pdf"] > 0.0
    assert valid.mean() >= 0.999 and st.kernel_vgprs > 0
    assert np.array_equal(got["light"], want["texel"]), "the texel the draws pick"
    assert np.array_equal(got["rng_state"], want["rng_state"]), "four draws"
    both = valid & want["valid"]
    err_d = float(np.abs(got["direction"][both] - want["direction"][both]).max())
    assert err_d <= 1e-12
    assert np.all(np.isinf(got["distance"][valid])) and not got["distance"][~valid].any() and not got["direction"][~valid].any()
    d = np.ascontiguousarray(got["direction"][valid])
    looked, pst = scene.environment_pdf(np.zeros_like(d), d, want=("pdf", "light"), variant=1, stats=True)
    assert not np.isnan(looked["pdf"]).any() and (looked["pdf"] >= 0.0).all() and pst.kernel_vgprs > 0
    e, u, v = E.coords(d, R)
    if cdf is not None:
        # the tables' factor of the texel the sampler's own lookup names -- the drawn one on nearly all samples -- over the
        # restated Jacobian; sqrt(1 - e_y^2) is the one ill-conditioned term: its relative error is that of e_y^2 over 1 - e_y^2
        limit = 64.0 * EPS * (1.0 + 1.0 / (1.0 - e[:, 1] * e[:, 1]))
        same = looked["light"] == got["light"][valid]
        assert same.mean() >= 0.999, "the direction lies in the texel drawn"
        j, i = np.divmod(got["light"][valid].astype(np.int64), w)
        pj = cdf[0][j] - np.where(j > 0, cdf[0][np.maximum(j - 1, 0)], 0.0)
        pi = cdf[1][j, i] - np.where(i > 0, cdf[1][j, np.maximum(i - 1, 0)], 0.0)
        pdf = ((pj * pi) * (float(w) * float(h))) / (((2.0 * PI) * PI) * np.sqrt(1.0 - e[:, 1] * e[:, 1]))
        err_p = np.abs(got["pdf"][valid][same] / pdf[same] - 1.0)
        err_q = np.abs(looked["pdf"] / got["pdf"][valid] - 1.0)
        print(f"{label}: {st.kernel_vgprs} VGPRs (sampler), {pst.kernel_vgprs} (density); direction {err_d:.3g}; pdf against the tables "
              f"{err_p.max():.3g} relative ({float((err_p / limit[same]).max()):.3g} of its bound), against environment_pdf {err_q.max():.3g} "
              f"({float((err_q / limit).max()):.3g} of its bound), bit-equal {np.mean(bits(looked['pdf']) == bits(got['pdf'][valid])):.4f}; "
              f"smallest 1 - e_y^2 {float((1.0 - e[:, 1] * e[:, 1]).min()):.3g}")
        assert np.all(err_p <= limit[same])
        assert np.all(err_q[same] <= limit[same])
        keep = texel_is_far_from_an_edge(w, h, e, u, v)
    else:
        assert np.all(got["light"] == -1) and np.all(looked["light"] == -1)
        uniform = bits(np.full(n, 1.0 / (4.0 * PI)))
        assert np.array_equal(bits(got["pdf"]), uniform) and np.array_equal(bits(looked["pdf"]), uniform[:len(d)])
        print(f"{label}: {st.kernel_vgprs} VGPRs (sampler), {pst.kernel_vgprs} (density); direction {err_d:.3g}")
        keep = None
    return got, valid, d, e, keep


def check_emitted(scene, got, valid, d, keep):
    assert keep.mean() >= 0.99
    along = emitted_along(scene, d, variant=1)
    assert np.array_equal(bits(along[keep]), bits(got["emitted"][valid][keep])), "the value is the lookup of the direction"


@pytest.mark.parametrize("kw", PLACEMENTS)
@pytest.mark.parametrize("name", sorted(SAMPLER_MAPS))
def test_samples_in_the_fast_build(name, kw):
    img = SAMPLER_MAPS[name]()
    k, R = placed(kw)
    scene = sampler_scene(img, **kw)
    got, valid, d, e, keep = check_sampler(f"{name} {sorted(kw)}", scene, img, k, R)
    check_emitted(scene, got, valid, d, keep)
    if name == "zero row 3x2":
        assert np.all(got["light"] < 3), "zero-weight texels are never drawn"
    if name == "1x1":
        assert np.all(got["light"] == 0) and np.all(got["pdf"] > 0.0)


def test_the_uniform_fallback_in_the_fast_build():
    scene = open_scene(lambda s: dict(texture=s.CheckerTexture(0.4, s.SolidColor((1, 1, 1)), s.SolidColor((0.1, 0.1, 0.1))), rotation=TILT))
    assert not scene.environment()["has_distribution"]
    got, valid, d, e, _ = check_sampler("uniform fallback", scene, None, np.ones(3), TILT)
    assert valid.all()
    check_emitted(scene, got, valid, d, checker_is_stable(1.0 / 0.4, e))
    assert np.max(np.abs(got["direction"].mean(axis=0))) < 5.0 / np.sqrt(3.0 * N_BITS), "uniform over the sphere"


@pytest.mark.parametrize("rows", [0, 1])
def test_both_sides_of_the_cap_of_the_staged_marginal_table_in_the_fast_build(rows):
    h = rt._lib.env_lds_rows() + rows
    img = float_map(2, h, seed=61)
    img[-1] *= 1e6            # the last row, at a pole, is drawn often: 1 - e_y^2 is smallest there
    img[h // 2] *= 300.0
    scene = sampler_scene(img)
    got, valid, d, e, keep = check_sampler(f"{h} rows", scene, img, np.ones(3), np.eye(3))
    check_emitted(scene, got, valid, d, keep)
    rows_drawn = got["light"] // 2
    assert np.sum(rows_drawn == h - 1) > 100 and np.sum(rows_drawn == h // 2) > 100 and len(np.unique(rows_drawn)) > 500


@pytest.mark.parametrize("name", ["sun 8x4", "zero row 3x2"])
def test_counts_and_the_estimate_of_the_integral_in_the_fast_build(name):
    """Statements about the distribution: they hold for any correct build."""
    img = SAMPLER_MAPS[name]()
    h, w = img.shape[:2]
    scene = sampler_scene(img, intensity=TINT, rotation=TILT)
    n = 65536
    got = scene.sample_environment(np.zeros((n, 3)), seed=SEED + 1, variant=1, want=("light", "pdf", "emitted"))
    marginal, conditional = scene.environment_cdf()
    P = (np.diff(marginal, prepend=0.0)[:, None] * np.diff(conditional, axis=1, prepend=0.0)).reshape(-1)
    P[np.repeat(np.diff(marginal, prepend=0.0) == 0.0, w)] = 0.0
    counts = np.bincount(got["light"], minlength=w * h)
    sigma = np.sqrt(n * P * (1.0 - P))
    assert np.all(np.abs(counts - n * P) <= 5.0 * sigma), "every texel within 5 binomial standard deviations"
    assert np.all(counts[P == 0.0] == 0), "zero-weight texels are never drawn"
    assert not np.isnan(got["pdf"]).any() and not np.isnan(got["emitted"]).any() and (got["pdf"] >= 0.0).all()
    valid = got["pdf"] > 0.0
    assert valid.mean() >= 0.999
    ratio = np.where(valid[:, None], got["emitted"] / np.where(valid, got["pdf"], 1.0)[:, None], 0.0)
    mean, err = ratio.mean(axis=0), ratio.std(axis=0, ddof=1) / np.sqrt(n)
    exact = E.integral(img, TINT)
    print(f"{name}: mean(emitted / pdf) {mean}, exact {exact}, standard errors {err}")
    assert np.all(np.abs(mean - exact) <= 5.0 * err)
