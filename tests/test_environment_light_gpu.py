"""The environment as a light of direct="mis" on the device (Scene.EnvironmentLight; include/rtow.h states the estimator under
rt_scene_path_advance_direct): the strict build against the restatement from public calls (tests/environment_light_restated.py)
bounce by bounce and bit for bit, the three routes as one estimator, "off is off", both sides of the staged table's cap, the
estimator's expectation and what it is worth, and the fast build.  Every frame and ray set is 16 x 16 camera rays, except the cap
test (4096 rays, so that its two rows are picked often enough) and the estimator checks (512 points x 64 batches)."""
import functools

import numpy as np
import pytest
import torch

import environment_light_restated as elr
import film_direct_restated as fdr
import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib
from query_helpers import bits
from test_environment_gpu import DEPTH, H, SEED, W, float_map, route_world, sun_map

pytestmark = pytest.mark.gpu

ALL = tuple(_lib.ADVANCE_DIRECT_OUTPUTS)
SPP = 4
BIT = rt.SCENE_FLAG_ENVIRONMENT_LIGHT
TILT = [[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]   # a quarter turn about the vertical, exact in fp64: the sun map's sun stays above the ground
FOG_BOX = ((-1.6, -0.5, -0.6), (1.6, 0.9, 2.2))
RULE = (4, 2, 0.35)   # the adaptive film's rule of tests/test_film_direct_gpu.py, cap 8


def zero_row_map():
    img = float_map(3, 2, seed=52)
    img[1] = 0.0
    return img


def lit(scene, chance, **environment):
    """``scene`` with another sky (``environment``: the arguments of Scene.Environment) and the environment as a light."""
    if environment:
        scene.Environment(**environment)
    scene.EnvironmentLight(chance)
    scene.Commit()
    return scene


def fog_world(fog=True):
    """route_world("list")'s objects inside a box of thin fog, so that paths scatter in it and shadow rays cross it; ``fog=False``:
    the twin without the fog, for the shadow rays no medium meets."""
    s = rt.Scene()
    grey, metal = s.Lambertian((0.6, 0.55, 0.5)), s.Metal((0.8, 0.8, 0.7), 0.1)
    items = [s.Sphere((0, -100.5, 0), 100.0, s.Lambertian((0.4, 0.5, 0.3))), s.Sphere((0, 0, 0), 0.5, grey), s.Sphere((1.1, 0, 0.2), 0.5, metal),
             s.Translate(s.MakeBox((-0.3, 0, -0.3), (0.3, 0.6, 0.3), grey), (0.2, -0.5, 1.2))]
    if fog:
        items.append(s.ConstantMedium(s.MakeBox(*FOG_BOX, grey), 0.6, (0.9, 0.9, 0.9)))
    s.SetWorld(s.HittableList(items))
    s.Camera((0.5, 1.2, 4.5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.05, 4.5, 0.0, 1.0, background=(0, 0, 0))
    return lit(s, 0.5, image=sun_map(), rotation=TILT)


WORLDS = {
    "list": lambda: lit(route_world("list"), 0.5, image=sun_map(), rotation=TILT),            # no lamp: c_e = 1 whatever the chance
    "bvh": lambda: lit(route_world("bvh"), 0.5, image=sun_map(), rotation=TILT),
    "moving mesh": lambda: lit(route_world("moving mesh"), 0.5, image=sun_map(), rotation=TILT),
    "lamp 0.5": lambda: lit(route_world("lamp"), 0.5, image=sun_map(), rotation=TILT),
    "lamp 1.0": lambda: lit(route_world("lamp"), 1.0, image=sun_map(), rotation=TILT),
    "checker sky": lambda: (lambda s: lit(s, 0.5, texture=s.CheckerTexture(0.4, s.SolidColor((3, 3, 3)), s.SolidColor((0.1, 0.1, 0.1))),
                                          rotation=TILT))(route_world("list")),
    "zero row": lambda: lit(route_world("list"), 0.5, image=zero_row_map()),
    "fog": fog_world,
}


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


def camera_rays(scene, width=W, height=H):
    o, d, tm, states = fdr.camera_rays_from(scene, fdr.seeded_states(SEED, width, height), width, height)
    n = width * height
    return dict(origin=o, direction=d, time=tm, rng_state=states, throughput=np.ones((n, 3)), ray_id=np.arange(n, dtype=np.int32),
                scatter_pdf=np.zeros(n))


def advance(scene, live, radiance, strategy, sample, variant=0):
    return scene.path_advance_direct(live["origin"], live["direction"], times=live["time"], rng_state=live["rng_state"],
                                     throughput=live["throughput"], ray_id=live["ray_id"], radiance=radiance, scatter_pdf=live["scatter_pdf"],
                                     strategy=strategy, sample=sample, variant=variant, want=ALL, stats=True)


def same(got, want):
    for k in ALL:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    return True


def fog_shadows(scene, got, before, after, seen):
    """What the restatement cannot do from public calls: a shadow ray that meets the fog draws from the path's stream.  For a ray
    whose stream the device left where the sample left it, nothing was drawn: the fog said no without a draw (its boundary lies
    outside the interval), and the answer is the twin's without the fog.  For a ray whose stream moved, it moved by exactly one
    draw (one medium, tested once), a blocker of the twin still blocks, and otherwise the device's own decision is taken -- read
    off its radiance row, which then has to be the restated L to the bit, or untouched."""
    twin = world_without_fog()

    def answer(P, direction, distance, tt, rows, streams):
        clear = ~twin.occluded(*scene.shadow_rays(P, direction, distance, tt))
        device = got["rng_state"][rows]
        drew = (device != streams).any(axis=1)
        for k in np.flatnonzero(drew):
            rng = rt.Rng.from_state(streams[k])
            rng.uniform()
            assert np.array_equal(np.asarray(rng.state(), dtype=np.uint32), device[k]), "exactly one draw from the path's own stream"
        ids = got["ray_id"][rows]
        added = (bits(after[ids]) != bits(before[ids])).any(axis=1)
        assert not (added & ~clear).any(), "what blocks without the fog blocks with it"
        visible = np.where(drew, added, clear)
        seen["fog draws"] += int(drew.sum())
        seen["fog blocked"] += int((drew & clear & ~added).sum())
        return visible, device
    return answer


@functools.lru_cache(maxsize=None)
def world_without_fog():
    return fog_world(fog=False)


def bounce_by_bounce(scene, live, depth, strategy=1, fog=False):
    """Check A: after every one of ``depth`` calls the radiance, every survivor array, the streams, scatter_pdf and the shadow
    statistics against the restatement.  Returns the restatement's bookkeeping, summed."""
    n = len(live["ray_id"])
    radiance, want_radiance = np.zeros((n, 3)), np.zeros((n, 3))
    seen = {k: 0 for k in ("cast", "reached", "sky_picks", "table_picks", "sky_ends", "lamp_ends", "dark_samples", "isotropic", "fog draws", "fog blocked")}
    seen["lamp_weights"], seen["sky_rows"] = [], []
    for bounce in range(depth):
        sample = bounce < depth - 1
        before = radiance.copy()
        got, st = advance(scene, live, radiance, strategy, sample)
        shadows = fog_shadows(scene, got, before, radiance, seen) if fog else None
        want, want_radiance, told = elr.restated(scene, live, want_radiance, strategy, sample, shadows=shadows)
        assert len(got["ray_id"]) == len(want["ray_id"]) == st.scattered, bounce
        assert same(got, want), bounce
        assert np.array_equal(bits(radiance), bits(want_radiance)), bounce
        assert st.shadow_rays == told["cast"] and st.shadow_reached == told["reached"], (bounce, st.shadow_rays, st.shadow_reached, told)
        if not sample:
            assert st.shadow_rays == 0 and not got["scatter_pdf"].any()
        for k, v in told.items():
            seen[k] = seen[k] + (list(v) if isinstance(seen[k], list) else v)
        live = {k: np.ascontiguousarray(a) for k, a in got.items()}
    print({k: (len(v) if isinstance(v, list) else v) for k, v in seen.items()})
    assert radiance.any() and (radiance >= 0).all()
    return seen


# ---- A. bounce by bounce against the restatement, bit for bit ----
@pytest.mark.parametrize("name,strategy", [("list", 1), ("bvh", 1), ("moving mesh", 1), ("lamp 0.5", 0), ("lamp 0.5", 1), ("lamp 1.0", 1),
                                           ("checker sky", 1), ("zero row", 1), ("fog", 1)])
def test_every_bounce_is_the_restatement(name, strategy):
    scene = world(name)
    lamps = scene.info()["n_lights"]
    told = scene.environment_light()
    assert scene.flags() & BIT and told["effective"] == (told["chance"] if lamps else 1.0)
    seen = bounce_by_bounce(scene, camera_rays(scene), DEPTH, strategy, fog=name == "fog")
    assert seen["sky_picks"] > 0, "environment picks"
    assert seen["sky_ends"] > 0, "a miss with q > 0"
    assert seen["reached"] > 0 and seen["cast"] - seen["reached"] > 0, "shadow rays both reached and blocked"
    if name == "lamp 0.5":
        assert seen["table_picks"] > 0 and seen["lamp_ends"] > 0, "table picks, and a lamp end with q > 0"
    elif name == "lamp 1.0":
        assert lamps == 1 and seen["table_picks"] == 0, "chance 1: no table sample is drawn"
        assert seen["lamp_ends"] > 0 and all(w == 1.0 for w in seen["lamp_weights"]), "every lamp end has w = 1"
    else:
        assert lamps == 0 and seen["table_picks"] == 0 and seen["lamp_ends"] == 0
    if name == "checker sky":
        assert not scene.environment()["has_distribution"], "no tables: the uniform fallback"
    if name == "zero row":
        assert seen["dark_samples"] > 0, "samples with C == 0"
    if name == "fog":
        assert seen["isotropic"] > 0 and seen["fog draws"] > 0, "isotropic scatter, and shadow rays that draw from the path's stream"


def test_the_setter_is_refused_while_a_render_is_in_flight():
    scene = rt.builtin_scene(0, 0, 64, 64)
    film = rt.Film(64, 64)
    film.launch(scene, film.params(8, variant=0))
    with pytest.raises(rt.RtowError, match="in flight"):
        scene.EnvironmentLight(0.5)
    with pytest.raises(rt.RtowError, match="in flight"):
        scene.EnvironmentLight(float("nan"))   # the order of include/rtow.h: the state before the chance
    film.finish()
    scene.EnvironmentLight(0.5)


# ---- B. the routes are one estimator ----
def to_device(a):
    return torch.from_numpy(np.array(a)).cuda()


def through_every_route(scene, variant=0):
    """(Scene.radiance(direct="mis") of the first sample's camera rays, the direct film's pixels): PathBatch.run, the radiance
    query on numpy arrays and on torch tensors, and the film are checked against each other on the way."""
    first = camera_rays(scene)
    o, d, tm, states = (first[k] for k in ("origin", "direction", "time", "rng_state"))
    mis = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, variant=variant, direct="mis", want=("radiance", "rng_state"))
    dev = scene.radiance(to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states.view(np.int32)), samples=1, max_depth=DEPTH,
                         variant=variant, direct="mis", want=("radiance", "rng_state"))
    assert np.array_equal(bits(dev["radiance"].cpu().numpy()), bits(mis["radiance"])), "the numpy and the torch call path"
    assert np.array_equal(dev["rng_state"].cpu().numpy().view(np.uint32), mis["rng_state"])
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states.view(np.int32)), variant=variant,
                         direct="mis")
    run = batch.run(DEPTH)
    torch.cuda.synchronize()
    assert np.array_equal(bits(run.cpu().numpy()), bits(mis["radiance"])), "PathBatch(direct='mis').run"
    film = rt.Film(W, H)
    film.render(scene, SPP, direct="mis", max_depth=DEPTH, seed=SEED, variant=variant)
    return mis["radiance"], film.download()


@pytest.mark.parametrize("name", ["list", "bvh", "moving mesh"])
def test_the_routes_are_one_estimator(name):
    scene = world(name)
    mis, frame = through_every_route(scene)
    want = fdr.Frame(scene, W, H, SEED).launch(SPP, DEPTH, direct=True)      # Scene.radiance(direct="mis"), sample by sample
    assert np.array_equal(bits(frame), bits(want.pixels())) and want.shadow_rays > want.shadow_reached > 0
    film = rt.Film(W, H)
    film.set_adaptive(*RULE)
    film.render(scene, 8, direct="mis", max_depth=DEPTH, seed=SEED, variant=0)
    adaptive = fdr.Frame(scene, W, H, SEED).launch(8, DEPTH, rule=RULE, direct=True)
    assert np.array_equal(film.sample_counts(), adaptive.counts()) and np.array_equal(bits(film.download()), bits(adaptive.pixels()))
    # the fold of single calls is that radiance too (A pins each call; this pins their sum to the one-kernel routes)
    live, radiance = camera_rays(scene), np.zeros((W * H, 3))
    for bounce in range(DEPTH):
        got, _ = advance(scene, live, radiance, 1, bounce < DEPTH - 1)
        live = {k: np.ascontiguousarray(a) for k, a in got.items()}
    assert np.array_equal(bits(radiance), bits(mis))


# ---- C. off is off ----
def test_chance_zero_is_a_scene_that_never_called_the_setter():
    """What test_the_routes_with_light_samples_agree_under_an_environment pins today: the same bits through all three routes."""
    never, zero = route_world("lamp"), lit(route_world("lamp"), 0.0)
    assert zero.flags() == never.flags() and not zero.flags() & BIT
    a, b = through_every_route(never), through_every_route(zero)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and a[0].any()


@pytest.mark.parametrize("name", ["list", "lamp 0.5"])
def test_with_the_bit_one_bounce_is_the_plain_radiance(name):
    scene = world(name)
    first = camera_rays(scene)
    o, d, tm, states = (first[k] for k in ("origin", "direction", "time", "rng_state"))
    plain = scene.radiance(o, d, times=tm, rng_state=states, samples=3, max_depth=1, want=("radiance", "rng_state"))
    mis = scene.radiance(o, d, times=tm, rng_state=states, samples=3, max_depth=1, direct="mis", want=("radiance", "rng_state"))
    assert np.array_equal(bits(mis["radiance"]), bits(plain["radiance"])) and np.array_equal(mis["rng_state"], plain["rng_state"]) and plain["radiance"].any()


def test_with_the_bit_and_without_lamps_the_samples_do_something():
    scene = world("list")
    first = camera_rays(scene)
    o, d, tm, states = (first[k] for k in ("origin", "direction", "time", "rng_state"))
    plain = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH)["radiance"]
    mis, st = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=DEPTH, direct="mis", stats=True)
    assert scene.info()["n_lights"] == 0 and st.shadow_rays > 0
    assert not np.array_equal(bits(plain), bits(mis["radiance"]))


# ---- D. both sides of the staged table's cap ----
@pytest.mark.parametrize("rows", [0, 1])
def test_both_sides_of_the_cap_of_the_staged_marginal_table(rows):
    h = _lib.env_lds_rows() + rows
    img = float_map(2, h, seed=61)
    img[-1] *= 1e6            # the last row -- the one beyond the cap where there is one -- is drawn often, although it lies at a pole
    img[h // 2] *= 300.0
    scene = lit(route_world("list"), 0.5, image=img)
    assert scene.environment_cdf()[0].shape == (h,)
    seen = bounce_by_bounce(scene, camera_rays(scene, 64, 64), 2)
    picked = np.asarray(seen["sky_rows"]) // 2
    print(f"cap + {rows}: {len(picked)} environment samples, last row {np.sum(picked == h - 1)}, middle row {np.sum(picked == h // 2)}")
    assert np.sum(picked == h - 1) > 100 and np.sum(picked == h // 2) > 100
    assert seen["sky_ends"] > 0 and seen["dark_samples"] > 0, "a miss with q > 0; the pole's samples leave below the ground: C == 0"


# ---- E. unbiased, and worth it ----
def sun_ground():
    """The scene of tests/test_environment_gpu.py::test_sampling_the_sun_beats_finding_it_by_scattering -- a Lambertian ground and an
    occluding box under scene 15's sky reduced to 64 x 32, 512 points beside the box -- with the environment as a light."""
    sky = rt.sky_demo_scene(1, 16, 16).environment()["image"]
    small = sky.reshape(32, 4, 64, 4, 3).mean(axis=(1, 3)).astype(np.float32)
    s = rt.Scene()
    ground = s.Quad((-20, 0, -20), (40, 0, 0), (0, 0, 40), s.Lambertian((0.7, 0.7, 0.7)))
    s.SetWorld(s.HittableList([ground, s.MakeBox((-1, 0, -1), (1, 2, 1), s.Lambertian((0.3, 0.3, 0.3)))]))
    s.Camera((0, 5, 12), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, background=(0, 0, 0))
    s.Environment(image=small)
    s.EnvironmentLight(1.0)
    s.Commit()
    n = 512
    rng = np.random.default_rng(7)
    target = np.stack([rng.uniform(-6, 6, 2 * n), np.zeros(2 * n), rng.uniform(-6, 6, 2 * n)], axis=-1)
    target = target[(np.abs(target[:, 0]) > 1.2) | (np.abs(target[:, 2]) > 1.2)][:n]
    o = np.ascontiguousarray(target + np.array((0.0, 6.0, 0.0)))
    d = np.ascontiguousarray(np.broadcast_to((0.0, -1.0, 0.0), (n, 3)))
    return s, o, d


def mean_and_error(x):
    """Per batch the mean over the rays of r + g + b; over the batches its mean and standard error."""
    lum = x.sum(axis=-1).mean(axis=1)
    return lum.mean(), lum.std(ddof=1) / np.sqrt(len(lum))


def sun_ground_estimates(variant=0, batches=64):
    """(A, B, F) as (mean, standard error): Scene.radiance, the host-composed next-event estimator of the test named above, and
    Scene.radiance(direct="mis") in the given build; two bounces."""
    s, o, d = sun_ground()
    n = len(o)
    a = np.stack([s.radiance(o, d, samples=1, max_depth=2, first_sequence=k * n)["radiance"] for k in range(batches)])
    f = np.stack([s.radiance(o, d, samples=1, max_depth=2, first_sequence=k * n, direct="mis", variant=variant)["radiance"] for k in range(batches)])
    b = []
    for k in range(batches):
        hit = s.path_step(o, d, first_sequence=k * n, want=("status", "attenuation", "origin", "normal", "material", "rng_state"))
        smp = s.sample_environment(hit["origin"], normals=hit["normal"], materials=hit["material"], rng_state=hit["rng_state"],
                                   want=("direction", "distance", "contribution"))
        lit_ = ~s.occluded(*s.shadow_rays(hit["origin"], smp["direction"], smp["distance"])) & (smp["distance"] > 0.0)
        b.append(np.where(lit_[:, None], hit["attenuation"] * smp["contribution"], 0.0))
    return mean_and_error(a), mean_and_error(f), mean_and_error(np.stack(b))


def test_sampling_the_sun_inside_the_estimator_is_unbiased_and_beats_scattering():
    (ma, ea), (mf, ef), (mb, eb) = sun_ground_estimates()
    print(f"sun ground: A (radiance) {ma:.5f} +- {ea:.5f}, B (host-composed) {mb:.5f} +- {eb:.5f}, F (direct='mis', environment light) {mf:.5f} +- {ef:.5f}; "
          f"e_A / e_F {ea / ef:.2f}, e_A / e_B {ea / eb:.2f}")
    assert abs(mf - ma) <= 5.0 * np.hypot(ef, ea)
    assert abs(mf - mb) <= 5.0 * np.hypot(ef, eb)
    assert ef < ea, "the test that fails without the feature: without it F is A's estimator"


@pytest.mark.parametrize("name", ["lamp 0.5", "lamp 1.0"])
def test_the_two_shares_and_the_per_emitter_weights_are_unbiased_together(name):
    """Lamp and sky together, eight bounces, 64 batches of 16 samples a camera ray.  At chance 1 the one-mixture weights would be
    biased (the lamp's light would be weighted as if table samples were still taken)."""
    scene = world(name)
    first = camera_rays(scene)
    o, d, tm = (first[k] for k in ("origin", "direction", "time"))
    n, batches = len(o), 64
    a = np.stack([scene.radiance(o, d, times=tm, samples=16, max_depth=8, seed=77, first_sequence=k * n)["radiance"] for k in range(batches)])
    f = np.stack([scene.radiance(o, d, times=tm, samples=16, max_depth=8, seed=78, first_sequence=k * n, direct="mis")["radiance"] for k in range(batches)])
    (ma, ea), (mf, ef) = mean_and_error(a), mean_and_error(f)
    print(f"{name}: A {ma:.5f} +- {ea:.5f}, F {mf:.5f} +- {ef:.5f}, |F - A| / combined {abs(mf - ma) / np.hypot(ef, ea):.2f}")
    assert abs(mf - ma) <= 5.0 * np.hypot(ef, ea)


def test_the_shadow_rays_through_fog_are_unbiased():
    """The fog world, eight bounces, 64 batches of 16 samples a camera ray, F against A within five combined standard errors: the
    medium's decision about a shadow ray, which check A can only take from the device, is held to the expectation here."""
    scene = world("fog")
    first = camera_rays(scene)
    o, d, tm = (first[k] for k in ("origin", "direction", "time"))
    n, batches = len(o), 64
    a = np.stack([scene.radiance(o, d, times=tm, samples=16, max_depth=8, seed=77, first_sequence=k * n)["radiance"] for k in range(batches)])
    f, cast, reached = [], 0, 0
    for k in range(batches):
        out, st = scene.radiance(o, d, times=tm, samples=16, max_depth=8, seed=78, first_sequence=k * n, direct="mis", stats=True)
        f.append(out["radiance"])
        cast, reached = cast + st.shadow_rays, reached + st.shadow_reached
    (ma, ea), (mf, ef) = mean_and_error(a), mean_and_error(np.stack(f))
    print(f"fog: A {ma:.5f} +- {ea:.5f}, F {mf:.5f} +- {ef:.5f}, |F - A| / combined {abs(mf - ma) / np.hypot(ef, ea):.2f}; {reached} of {cast} shadow rays reached the sky")
    assert abs(mf - ma) <= 5.0 * np.hypot(ef, ea)
    assert 0 < reached < cast and ef < ea


# ---- F. the fast build ----
@pytest.mark.parametrize("name", ["list", "lamp 0.5", "moving mesh"])
def test_the_fast_build_agrees_with_itself_through_every_route(name):
    """Within the build the numpy and the torch path, PathBatch.run and the radiance query are the same bits (through_every_route);
    against the strict build the yardstick is per ray: the share of rays within 1e-9 relative is printed, the paths that take
    another branch under contraction aside."""
    scene = world(name)
    fast, frame = through_every_route(scene, variant=1)
    strict, _ = through_every_route(scene, variant=0)
    scale = np.maximum(np.abs(strict), 1e-300)
    close = (np.abs(fast - strict) / scale <= 1e-9).all(axis=1)
    worst = np.max(np.abs(fast - strict)[close] / scale[close]) if close.any() else 0.0
    print(f"fast against strict, {name}: {close.mean():.4f} of {len(close)} rays within 1e-9 relative, the worst of those {worst:.3g}; bit-equal "
          f"{np.mean((bits(fast) == bits(strict)).all(axis=1)):.4f}")
    assert fast.any() and np.isfinite(frame).all()


def test_the_fast_build_is_unbiased_on_the_sun_ground():
    (ma, ea), (mf, ef), _ = sun_ground_estimates(variant=1, batches=64)
    print(f"sun ground, fast build: A {ma:.5f} +- {ea:.5f}, F {mf:.5f} +- {ef:.5f}")
    assert abs(mf - ma) <= 5.0 * np.hypot(ef, ea)
