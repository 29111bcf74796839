"""Path advances with light samples on the device (rt_scene_path_advance_direct, Scene.path_advance_direct, PathBatch(direct="mis")).
Without lights the call is the plain advance bit for bit; with lights the strict build is a numpy restatement built from the public
calls (path_step, sample_lights, light_pdf, occluded(*shadow_rays), rt.scatter_pdf), one operation at a time in the header's order,
after every one of six bounces; PathBatch(direct="mis").run is the fold of those calls; and the fold is an estimator of what
Scene.radiance estimates."""
import functools
import math

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib

import light_restated as lr
from light_worlds import QUAD, TRIANGLE, SPHERE, MSPHERE, many_lights_world, no_lights_world, single_kind_world
from query_helpers import bits
from triangle_meshes import icosphere

pytestmark = pytest.mark.gpu

ALL = tuple(_lib.ADVANCE_DIRECT_OUTPUTS)
PLAIN = tuple(_lib.ADVANCE_OUTPUTS)
SEED = 1984
N = 1000        # four workgroups, the last one partial
BOUNCES = 6
CAP = _lib.light_lds_rows()

LAMP = ((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))
BALL = ((1.2, 1.5, 0.3), 0.25)
SHADE = ((-0.1, 0.5, -0.4), (1.0, 0.0, 0.0), (0.0, 0.0, 0.8))
FOG = ((0.0, 1.1, 0.0), 0.35)   # between the lamp and the floor, clear of the shade's plane


def lamp_scene(medium=None, fog=False):
    """The scene of the light sampling tests' estimator check: a checkered floor, a quad lamp, a ball lamp and a shade.  ``medium``:
    (centre, radius) of a ConstantMedium beside it all; ``fog``: a fog ball between the lamp and the floor."""
    s = rt.Scene()
    floor = s.Lambertian(s.CheckerTexture(0.5, s.SolidColor((0.8, 0.8, 0.8)), s.SolidColor((0.3, 0.5, 0.7))))
    items = [s.Quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), floor), s.Quad(*LAMP, s.DiffuseLight((8.0, 8.0, 8.0))),
             s.Sphere(*BALL, s.DiffuseLight((10.0, 6.0, 3.0))), s.Quad(*SHADE, s.Lambertian((0.5, 0.5, 0.5)))]
    if medium:
        items.append(s.ConstantMedium(s.Sphere(*medium, s.Lambertian((0.5, 0.5, 0.5))), 0.5, (0.9, 0.9, 0.9)))
    if fog:
        items.append(s.ConstantMedium(s.Sphere(*FOG, s.Lambertian((0.5, 0.5, 0.5))), 1.5, (0.9, 0.9, 0.9)))
    s.SetWorld(s.HittableList(items))
    s.Camera((0, 1, 6), (0, 1, 0), (0, 1, 0), 40.0, 1.0, 0.0, 6.0, background=(0, 0, 0))
    s.Commit()
    return s


def many_lights_over_a_floor(n_lights):
    """many_lights_world's lamps above a diffuse floor: light samples then pick rows beyond the part staged on chip."""
    s = rt.Scene()
    lamp = s.DiffuseLight(s.CheckerTexture(0.5, s.SolidColor((2.0, 1.0, 0.5)), s.SolidColor((0.5, 1.0, 2.0))))
    verts, faces = icosphere(2, 2.0)
    assert n_lights <= len(faces)
    mesh = s.TriangleMesh(verts + np.array([0.0, 3.0, 0.0]), faces[:n_lights], lamp)
    floor = s.Quad((-10, -1, -10), (20, 0, 0), (0, 0, 20), s.Lambertian((0.5, 0.5, 0.5)))
    s.SetWorld(s.HittableList([floor, mesh]))
    s.Camera((0, 0, 10), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0, background=(0, 0, 0))
    s.Commit()
    return s


# A small ball of fog far away and below the horizon: no shadow ray can meet it (they run from the floor to the lamps, a few units
# about the origin), and a path would have to leave the scene into a cone of 2e-7 steradians (restated() checks that none
# scatters inside it).  Its presence alone switches the occlusion search to its full form.
FAR_MEDIUM = ((400.0, -50.0, 0.0), 0.1)
WORLDS = {
    "lamp scene": lamp_scene,
    "quads": lambda: single_kind_world(QUAD)[0], "triangles": lambda: single_kind_world(TRIANGLE)[0],
    "spheres": lambda: single_kind_world(SPHERE)[0], "moving spheres": lambda: single_kind_world(MSPHERE)[0],
    "300 lights": lambda: many_lights_world(300)[0],
    "300 lights over a floor": lambda: many_lights_over_a_floor(300),
    "lamp scene beside a medium": lambda: lamp_scene(medium=FAR_MEDIUM),
}


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def rays(count=N):
    """Rays from around (0, 0.5, 6): three in four towards points on and under the floors, one in four towards the lamps above them,
    some up and away from everything; times in the shutter;
    seeded streams; one dead ray; one id outside the radiance array; every third ray (some of every kind above) carries a density
    into its first bounce, as if a bounce before had sent it."""
    g = np.random.default_rng(11)
    o = np.ascontiguousarray(np.array([0.0, 0.5, 6.0]) + g.uniform(-0.25, 0.25, size=(count, 3)))
    target = g.uniform((-2.5, -1.2, -2.5), (2.5, 0.2, 2.5), size=(count, 3))
    target[::4] = g.uniform((-2.0, 1.0, -2.0), (2.5, 3.0, 2.0), size=target[::4].shape)
    d = np.ascontiguousarray(target - o)
    d[::17] = g.uniform((-1.0, 0.5, 0.2), (1.0, 1.0, 1.0), size=d[::17].shape)   # behind and above the camera: they miss everything
    tm = np.ascontiguousarray(g.uniform(0.0, 1.0, size=count))
    states = lr.seeded_states(count, SEED)
    alive = np.ones(count, dtype=np.uint8)
    alive[3] = 0
    ids = np.arange(count, dtype=np.int32)
    ids[5] = count + 7
    q = np.where(np.arange(count) % 3 == 1, 0.25, 0.0)
    out = dict(origin=o, direction=d, time=tm, rng_state=states, throughput=np.ones((count, 3)), ray_id=ids, scatter_pdf=q, alive=alive)
    for a in out.values():
        a.setflags(write=False)
    return out


def restated(scene, live, radiance, strategy, sample, alive=None):
    """One call of rt_scene_path_advance_direct from the public calls, one IEEE operation at a time in the order of include/rtow.h:
    (the survivors' rows by output name, the radiance array afterwards).  Valid where no ray meets a medium: the shadow rays then
    draw nothing."""
    o, d, tm, states = live["origin"], live["direction"], live["time"], live["rng_state"]
    T, ids, q = live["throughput"], live["ray_id"], live["scatter_pdf"]
    n = len(ids)
    alive = np.ones(n, dtype=bool) if alive is None else alive != 0
    step = scene.path_step(o, d, times=tm, rng_state=states, want=tuple(_lib.STEP_OUTPUTS))
    status, m, nrm = step["status"], step["material"], step["normal"]
    after = radiance.copy()
    inside = (ids >= 0) & (ids < len(after))
    with np.errstate(all="ignore"):
        # the path ended
        ends = alive & (status != 2)
        lamp = ends & (status == 1) & (m == 3) & (q > 0)
        p_in = scene.light_pdf(o, d, times=tm, strategy=strategy)["pdf"]
        w = np.where(lamp, q / (q + p_in), 1.0)
        sel = ends & inside
        after[ids[sel]] = after[ids[sel]] + (T[sel] * step["emitted"][sel]) * w[sel][:, None]
        # the path scattered
        goes = alive & (status == 2)
        Tn = T * step["attenuation"]
        q_next = np.zeros(n)
        states_next = step["rng_state"].copy()
        shadow_rays = 0
        assert scene is not world("lamp scene beside a medium") or not (alive & (m == 4)).any(), "a path scattered inside the far medium"
        if sample and len(scene.lights()["kind"]):
            idx = np.flatnonzero(goes & ((m == 0) | (m == 4)))
            if len(idx):
                P, nn, tt = (np.ascontiguousarray(step[k][idx]) for k in ("origin", "normal", "time"))
                ls = scene.sample_lights(P, nn, np.ascontiguousarray(m[idx]), tt, np.ascontiguousarray(step["rng_state"][idx]), strategy=strategy)
                states_next[idx] = ls["rng_state"]
                C, s = ls["contribution"], ls["scatter_pdf"]
                p = scene.light_pdf(P, ls["direction"], times=tt, strategy=strategy)["pdf"]
                wl = np.where(p + s == 0, 0.0, p / (p + s))
                L = (Tn[idx] * C) * wl[:, None]
                cast = (C != 0).any(axis=1)
                shadow_rays = int(cast.sum())
                visible = np.zeros(len(idx), dtype=bool)
                if cast.any():
                    shadow = scene.shadow_rays(np.ascontiguousarray(P[cast]), np.ascontiguousarray(ls["direction"][cast]),
                                               np.ascontiguousarray(ls["distance"][cast]), np.ascontiguousarray(tt[cast]))
                    visible[cast] = ~scene.occluded(*shadow)
                add = visible & inside[idx]
                after[ids[idx][add]] = after[ids[idx][add]] + L[add]
                dn = step["direction"][idx]
                u = (1.0 / np.sqrt((dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]) + dn[:, 2] * dn[:, 2]))[:, None] * dn
                q_next[idx] = rt.scatter_pdf(m[idx], nn, u)
    out = {k: step[k][goes] for k in ("origin", "direction", "time", "t", "normal", "front_face", "material")}
    out.update(rng_state=states_next[goes], throughput=Tn[goes], ray_id=ids[goes], scatter_pdf=q_next[goes])
    return out, after, dict(cast=shadow_rays, lamp=int(lamp.sum()))


def same(got, want, keys=ALL):
    for k in keys:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    return True


def contiguous(rows):
    return {k: np.ascontiguousarray(a) for k, a in rows.items()}


def advance(scene, live, radiance, strategy, sample, alive=None, variant=0, want=ALL, stats=False):
    return scene.path_advance_direct(live["origin"], live["direction"], times=live["time"], rng_state=live["rng_state"],
                                     throughput=live["throughput"], ray_id=live["ray_id"], alive=alive, radiance=radiance,
                                     scatter_pdf=live["scatter_pdf"], strategy=strategy, sample=sample, variant=variant, want=want, stats=stats)


def to_device(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(name, tensor):
    a = tensor.cpu().numpy()
    return a.view(np.uint32) if name == "rng_state" else a


# ---- 1. without lights it is the plain advance ----
@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_without_lights_it_is_the_plain_advance_bit_for_bit(variant):
    scene = no_lights_world()
    r = {k: np.array(a[:257]) for k, a in rays().items()}
    r["ray_id"][5] = 300
    thr = np.ascontiguousarray(np.random.default_rng(3).uniform(0.25, 1.0, size=(257, 3)))
    plain_radiance, radiance = np.full((257, 3), 0.125), np.full((257, 3), 0.125)
    plain = scene.path_advance(r["origin"], r["direction"], times=r["time"], rng_state=r["rng_state"], throughput=thr, ray_id=r["ray_id"],
                               alive=r["alive"], radiance=plain_radiance, variant=variant, want=PLAIN)
    live = dict(r, throughput=thr)
    got, st = advance(scene, live, radiance, 1, True, alive=r["alive"], variant=variant, stats=True)
    assert 0 < len(plain["ray_id"]) < 256, "some paths end and some go on"
    assert same(got, plain, PLAIN) and np.array_equal(bits(radiance), bits(plain_radiance))
    assert not got["scatter_pdf"].any() and st.shadow_rays == 0 and st.shadow_reached == 0
    assert st.rays == 256 and st.scattered == len(plain["ray_id"])
    # the torch path: the same bits
    dev = {k: to_device(a) for k, a in live.items()}
    dev_radiance = torch.full((257, 3), 0.125, dtype=torch.float64, device="cuda")
    got_dev = advance(scene, dev, dev_radiance, 1, True, alive=dev["alive"], variant=variant)
    assert same({k: to_host(k, a) for k, a in got_dev.items()}, got)
    assert np.array_equal(bits(dev_radiance.cpu().numpy()), bits(radiance))


# ---- 2. the strict build is the restatement ----
# (the uniform strategy on two worlds: the table is read the same way, only the cumulative column differs)
@pytest.mark.parametrize("name,strategy", [(name, 1) for name in sorted(WORLDS)] + [("lamp scene", 0), ("300 lights over a floor", 0)])
def test_the_strict_build_is_the_restatement_after_every_bounce(name, strategy):
    scene = world(name)
    first = rays()
    live = {k: first[k] for k in ("origin", "direction", "time", "rng_state", "throughput", "ray_id", "scatter_pdf")}
    alive = first["alive"]
    radiance, want_radiance = np.zeros((N, 3)), np.zeros((N, 3))
    seen = dict(cast=0, lamp=0, missed=0)
    for bounce in range(BOUNCES):
        sample = bounce < BOUNCES - 1
        want, want_radiance, told = restated(scene, live, want_radiance, strategy, sample, alive)
        got, st = advance(scene, live, radiance, strategy, sample, alive=alive, stats=True)
        assert len(got["ray_id"]) == len(want["ray_id"]) == st.scattered, bounce
        assert same(got, want), bounce
        assert np.array_equal(bits(radiance), bits(want_radiance)), bounce
        assert st.shadow_rays == told["cast"] and st.shadow_reached <= st.shadow_rays
        if not sample:
            assert st.shadow_rays == 0 and not got["scatter_pdf"].any()
        seen["cast"] += told["cast"]
        seen["lamp"] += told["lamp"]
        live, alive = contiguous(got), None
    assert seen["lamp"] > 0, "some weighted lamps"
    if name != "300 lights":   # (lamps alone: nothing scatters there)
        assert seen["cast"] > 100, "and shadow rays"
    assert not radiance[3].any(), "the dead ray's row"
    assert radiance.any() and (radiance >= 0).all()


def test_the_worlds_of_test_2_have_what_it_says():
    first = rays()
    scene = world("lamp scene")
    step = scene.path_step(first["origin"], first["direction"], times=first["time"], rng_state=first["rng_state"], want=("status",))
    assert (step["status"] == 0).sum() > 20 and (step["status"] == 2).sum() > 200
    assert len(world("300 lights").lights()["kind"]) == 300 > CAP and len(world("300 lights over a floor").lights()["kind"]) == 300
    assert first["alive"][3] == 0 and first["ray_id"][5] >= N


# ---- 3. PathBatch(direct="mis").run is that fold ----
def loop_of_calls(scene, first, depth, strategy, variant=0, kill_after_first=None):
    live = {k: to_device(first[k]) for k in ("origin", "direction", "time", "rng_state")}
    n = live["origin"].shape[0]
    live.update(throughput=torch.ones((n, 3), dtype=torch.float64, device="cuda"), ray_id=torch.arange(n, dtype=torch.int32, device="cuda"),
                scatter_pdf=torch.zeros(n, dtype=torch.float64, device="cuda"))
    radiance = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    alive = None
    for bounce in range(depth):
        live = advance(scene, live, radiance, strategy, bounce < depth - 1, alive=alive, variant=variant,
                       want=("origin", "direction", "time", "rng_state", "throughput", "ray_id", "scatter_pdf"))
        live = {k: a.contiguous() for k, a in live.items()}
        alive = None
        if bounce == 0 and kill_after_first is not None:
            alive = (~kill_after_first(live["ray_id"].shape[0])).to(torch.uint8)
    return radiance.cpu().numpy()


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("name", ["lamp scene", "spheres"])
def test_path_batch_run_is_the_fold_of_single_calls(name, variant):
    scene, first, depth = world(name), rays(), 4
    want = loop_of_calls(scene, first, depth, 1, variant)
    o, d, tm, states = (to_device(first[k]) for k in ("origin", "direction", "time", "rng_state"))
    for check_every in (0, 3):
        batch = rt.PathBatch(scene, o, d, times=tm, rng_state=states, variant=variant, direct="mis", strategy=1)
        got = batch.run(depth, check_every=check_every)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), check_every
        assert "scatter_pdf" in batch._sides[0] and batch.throughput.shape == (N, 3)
    assert want.any()


def test_path_batch_killed_rows_add_nothing():
    scene, first, depth = world("lamp scene"), rays(), 4
    mask = lambda rows: torch.arange(rows, device="cuda") % 3 == 0   # noqa: E731
    want = loop_of_calls(scene, first, depth, 1, kill_after_first=mask)
    untouched = loop_of_calls(scene, first, depth, 1)
    o, d, tm, states = (to_device(first[k]) for k in ("origin", "direction", "time", "rng_state"))
    batch = rt.PathBatch(scene, o, d, times=tm, rng_state=states, direct="mis")
    batch.advance(1)
    after_one = batch.radiance.clone()
    killed_ids = batch.ray_id[:batch.live()][mask(batch.live())].long()
    batch.kill(mask(batch.live()))
    batch.advance(depth - 2)
    batch.advance(1, sample=False)
    got = batch.radiance.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(untouched))
    assert torch.equal(batch.radiance[killed_ids], after_one[killed_ids]), "a killed row adds nothing after its kill"


def test_path_batch_without_direct_is_as_it_was():
    scene, first = world("lamp scene"), rays()
    o, d, tm, states = (to_device(first[k]) for k in ("origin", "direction", "time", "rng_state"))
    batch = rt.PathBatch(scene, o, d, times=tm, rng_state=states)
    assert batch.direct is None and "scatter_pdf" not in batch._sides[0] and isinstance(batch._calls[0][0], _lib.PathAdvanceParams)
    want = scene.radiance(first["origin"], first["direction"], times=first["time"], rng_state=first["rng_state"], samples=1, max_depth=5)["radiance"]
    assert np.array_equal(bits(batch.run(5).cpu().numpy()), bits(want))


# ---- 4. the estimator ----
BATCHES = 16
SAMPLES = 4096   # per point and batch, as the light sampling tests' estimator check
FOG_SAMPLES = 12288   # see test_the_fold_estimates_what_radiance_estimates_through_fog
FOG_DEPTH = 4


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


def floor_points():
    xs = -1.4 + 0.4 * np.arange(8)
    o = np.ascontiguousarray(np.array([(x, 0.05, z) for x in xs for z in xs]))
    d = np.ascontiguousarray(np.tile([0.0, -1.0, 0.0], (64, 1)))
    return o, d


def mean_se(x):
    return x.mean(axis=0), x.std(axis=0, ddof=1) / math.sqrt(len(x))


def estimates(scene, depth, samples, first_bounce=None):
    """(A, M): BATCHES independent means per point of Scene.radiance and of PathBatch(direct="mis").run, ``samples`` paths a point each.
    ``first_bounce``: a list that receives each batch's radiance after the first advance alone."""
    o, d = floor_points()
    A = np.stack([scene.radiance(o, d, samples=samples, max_depth=depth, seed=100, first_sequence=64 * b)["radiance"] for b in range(BATCHES)])
    O = torch.from_numpy(np.repeat(o, samples, axis=0)).cuda()
    D = torch.from_numpy(np.repeat(d, samples, axis=0)).cuda()
    n = O.shape[0]
    M = []
    for b in range(BATCHES):
        batch = rt.PathBatch(scene, O, D, seed=300, first_sequence=n * b, direct="mis", strategy=1)
        if first_bounce is not None:
            batch.advance(1)
            first_bounce.append(batch.radiance.reshape(64, samples, 3).sum(dim=1).cpu().numpy())
            batch.advance(depth - 2)
            batch.advance(1, sample=False)
            radiance = batch.radiance
        else:
            radiance = batch.run(depth, check_every=0)
        M.append(radiance.reshape(64, samples, 3).mean(dim=1).cpu().numpy())
    return A, np.stack(M)


def test_the_fold_estimates_what_radiance_estimates():
    """Scene.radiance(max_depth=2) against PathBatch(direct="mis").run(2) on the scene, the 64 points, the 16 batches and the 4096
    samples of the light sampling tests' estimator check: within 5 combined standard errors at every point and channel, the combined
    standard error of the lit points under 2 % of their mean, and exactly nothing from the first bounce's light samples at the
    points in full shadow."""
    scene = lamp_scene()
    o, _ = floor_points()
    shadowed = np.array([in_full_shadow(np.array([p[0], 0.0, p[2]])) for p in o])
    assert 2 <= shadowed.sum() <= 16
    first = []
    A, M = estimates(scene, 2, SAMPLES, first)
    (a, sa), (m, sm) = mean_se(A), mean_se(M)
    lit = a.sum(axis=1) > 0.0
    combined = np.sqrt(sa ** 2 + sm ** 2)
    print("lit points", int(lit.sum()), "mean A", a[lit].mean(), "se A", sa[lit].mean(), "se M", sm[lit].mean(), "combined", combined[lit].mean(),
          "max |A-M| / se", np.nanmax(np.abs(a - m)[lit] / combined[lit]))
    assert np.all(np.abs(a - m) <= 5.0 * combined)
    assert combined[lit].mean() <= 0.02 * a[lit].mean()
    assert lit.sum() >= 40 and not lit[shadowed].any()
    assert not np.stack(first)[:, shadowed].any(), "a point in full shadow gets exactly nothing from the first bounce's light samples"
    assert np.abs(m[lit] / a[lit] - 1.0).mean() < 0.05


def test_the_fold_estimates_what_radiance_estimates_through_fog():
    """The same scene with a fog ball between the lamp and the floor, four bounces: shadow rays cross a ConstantMedium and draw from
    the path's own stream.  The rule is the same 5 combined standard errors and the same 2 % cap, and Scene.radiance alone stays
    within half of the cap.  Measured on an MI355X at 4096 samples a point and batch: the standard error of Scene.radiance alone
    is 0.00453 on a lit mean of 0.3033, 1.49 % (the fold's: 0.00107) -- above the half, so the samples are 3 x 4096 = 12288, where
    1.49 % / sqrt(3) = 0.86 % is expected."""
    scene = lamp_scene(fog=True)
    A, M = estimates(scene, FOG_DEPTH, FOG_SAMPLES)
    (a, sa), (m, sm) = mean_se(A), mean_se(M)
    lit = a.sum(axis=1) > 0.0
    combined = np.sqrt(sa ** 2 + sm ** 2)
    print("fog: lit points", int(lit.sum()), "mean A", a[lit].mean(), "se A", sa[lit].mean(), "se A / mean", sa[lit].mean() / a[lit].mean(),
          "se M", sm[lit].mean(), "combined", combined[lit].mean(), "max |A-M| / se", np.nanmax(np.abs(a - m)[lit] / combined[lit]))
    assert sa[lit].mean() <= 0.01 * a[lit].mean(), "Scene.radiance alone within half of the cap"
    assert np.all(np.abs(a - m) <= 5.0 * combined)
    assert combined[lit].mean() <= 0.02 * a[lit].mean()
