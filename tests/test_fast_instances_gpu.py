"""The fast build (variant=1, -ffp-contract=fast) of the affine and the moving instance kernels: the `_x` units and their second
pass, namespace rtow::moving, launchers `*_xm`.  The strict build of these kernels is pinned to the restatements bit for bit
(tests/test_transform_gpu.py, tests/test_motion_transform_gpu.py); here the same worlds, chains and designed rays go through
variant=1 against the same references.  The rule throughout: a decision on an input designed with a margin is exact; a value is
held to a bound that comes from conditioning or to a tolerance the project already commits to (each names its file); what rounding
may decide -- a rejection loop's comparison with 1, a medium's comparison of two lengths -- is left out by a margin computed from
the restatement on the CPU, whose share is asserted there; the measured worst is printed.  Every ray set is the existing one of
1500 designed rays, every frame 32 x 24."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import light_restated as lr
import motion_restated as mr
import test_motion_transform_gpu as mtg
import test_transform_gpu as tg
import transform_restated as tr
from frame_helpers import compare
from query_helpers import bits, centre_rays, dot3, uv_bound
from test_motion_transform_host import MOVING_CHAINS
from test_radiance_gpu import _share_that_differs, camera_rays
from test_reference_gpu import MEDIUM_REL
from test_transform_gpu import CHAINS, CHILDREN, N, RECORD, SEED, W, H

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
T_REL = 1e-12         # fast against strict on one leaf: tests/test_ray_query_gpu.py
NORMAL_ABS = 1e-12    # the premise of query_helpers.uv_bound
UNIT_ABS = 1e-14
WITHIN_FAST = 0.995   # of a frame's pixels within 1e-5: min_within_fast of tests/test_custom_scenes_gpu.py
EXTRA_SHARE = 8 / 768   # tests/test_radiance_gpu.py test_strict_and_fast_differ_no_more_often_than_the_render_kernels_do
KEEP, ACCUMULATE = rt.FLAG_KEEP_RNG_STATE, rt.FLAG_ACCUMULATE
STEP_OUTPUTS = ("status", "t", "origin", "material", "rng_state")


# ---- what rounding may decide, from the restatement alone (CPU) ----
def lambertian_margin(states, rows):
    """Lambertian::Scatter's random unit vector (tests/test_path_step_gpu.py restates it ray by ray): three draws a try, 2 * (a, b, c)
    - 1, until the squared length is below 1.  That sum of squares may contract.  Returns, for the rays of the mask ``rows`` that
    scatter from the streams ``states``, how near any candidate's squared length comes to 1 (inf for the other rays), and the
    streams after the loop."""
    rng = lr.Streams(states)
    pending = np.array(rows, dtype=bool)
    nearest = np.full(len(pending), np.inf)
    while pending.any():
        x, y, z = (2.0 * rng.uniform(pending) - 1.0 for _ in range(3))
        len2 = (x * x + y * y) + z * z
        nearest[pending] = np.minimum(nearest[pending], np.abs(len2 - 1.0)[pending])
        pending &= ~(len2 < 1.0)
    return nearest, rng.s


def medium_margin(ro, rd, states, density=2.0, tmin=0.001):
    """ConstantMedium::Hit over the box of tests/test_transform_gpu.py's "medium" child for the restated local rays: the two
    boundary hits from the slabs, the clip to tmin, the length inside times |d|, and -(1 / density) * log(u) with the stream's first
    draw (the float overload of log, as csrc/render.hip medium_draw).  Returns (the relative difference of the two lengths that are
    compared, inf where the ray never comes to the draw; does it scatter by this restatement)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (tg.BOX_LO - ro) / rd, (tg.BOX_HI - ro) / rd
    enter, leave = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    enter = np.maximum(enter, tmin)
    draws = enter < leave
    inside = (leave - np.maximum(enter, 0.0)) * np.sqrt(dot3(rd, rd))
    u = lr.Streams(states).uniform()
    hit_dist = (-1.0 / density) * np.log(u).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        rel = np.where(draws, np.abs(hit_dist - inside) / np.maximum(hit_dist, np.abs(inside)), np.inf)
    return rel, draws & (hit_dist <= inside)


def left_out(name, ro, rd, states):
    """The rays whose outcome rounding may decide, from the restated local rays and streams: (mask, restated streams after the
    step for a Lambertian child or None).  Asserts, on the CPU, that at most 1 % of the rays are left out."""
    miss = np.arange(len(ro)) % 4 == 3
    if name == "medium":
        rel, scatters = medium_margin(ro, rd, states)
        out, after = rel < 1e-9, None
        assert 0.3 < scatters[~miss].mean() < 1.0 and not scatters[miss].any(), "the restatement: some rays scatter in the fog, some pass"
    else:
        nearest, after = lambertian_margin(states, ~miss)   # the aimed rays hit a Lambertian child: all of them scatter
        out = nearest <= 1e-12
    assert out.mean() <= 0.01, out.mean()
    return out, after


@functools.lru_cache(maxsize=None)
def streams():
    s = lr.seeded_states(1500, SEED)
    s.setflags(write=False)
    return s


# ---- 1. a placed and a moved child ----
def check_child(label, name, A, B, o, d, ro, rd, tm, forward_points, forward_normals):
    """A: the scene with the child under its chain, asked in the fast build with the world rays; B: the child alone, asked in the
    strict build with the restated local rays -- the reference of the strict tests.
    The scattered origin's bound, 64 eps (|P| + |t d|), is held against (L P') + t_L with P' = o' + t d' formed in numpy from the
    restated local ray and the step's OWN t, not against the strict reference's origin: on a flat face t = (D - n . o') / (n . d')
    has the relative condition |n| |d'| / |n . d'| with respect to the local ray, the designed rays bound the barycentric margin and
    not that grazing angle, and the origin moves along the ray with t.  Measured on the MI355X: t differs by up to 2.2e-13 relative
    on the box and the icosahedron (inside T_REL), which alone moves the origin by up to 8.7 times the bound; with the step's t the
    worst origin is 0.028 of the bound.  t itself stays held to T_REL."""
    n = len(o)
    states = np.array(streams())
    out, after = left_out(name, ro, rd, states)
    keep = ~out
    kw = dict(times=tm, seed=SEED)
    got = A.intersect(o, d, want=RECORD + ("normal",), variant=1, **kw)
    want = B.intersect(ro, rd, want=RECORD + ("normal",), variant=0, **kw)
    step_a = A.path_step(o, d, times=tm, rng_state=states, variant=1, want=STEP_OUTPUTS)
    step_b = B.path_step(ro, rd, times=tm, rng_state=states, variant=0, want=STEP_OUTPUTS)
    hit = np.isfinite(want["t"])
    miss = np.arange(n) % 4 == 3

    def rel(a, b):
        return float(np.abs(a / b - 1.0).max()) if len(a) else 0.0

    if name == "medium":
        # the ray query draws from curand_init(SEED, k, 0), the streams the step is given: one decision for both
        for res, ref in ((got, want), (step_a, step_b)):
            assert np.array_equal(np.isfinite(res["t"][keep]), np.isfinite(ref["t"][keep]))
        assert np.array_equal(step_a["status"][keep], step_b["status"][keep]) and np.array_equal(step_a["rng_state"][keep], step_b["rng_state"][keep])
        fin = keep & np.isfinite(step_b["t"])
        worst = max(rel(step_a["t"][fin], step_b["t"][fin]), rel(got["t"][keep & hit], want["t"][keep & hit]))
        print(f"{label}: {out.sum()} of {n} rays left out; {fin.sum()} scatter in the fog, t differs by at most {worst:.3g} relative (bound {MEDIUM_REL + 1e-12:.3g})")
        assert 0.3 < hit[~miss].mean() < 1.0 and not hit[miss].any()
        assert worst <= MEDIUM_REL + 1e-12
        return dict(t=worst, left_out=out.mean())
    # decisions: exact, for every ray
    assert hit[~miss].all() and not hit[miss].any(), "the reference: the aimed rays hit, the others miss"
    assert np.array_equal(np.isfinite(got["t"]), hit), int(np.sum(np.isfinite(got["t"]) != hit))
    for key in ("front_face", "material"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(step_a["status"], step_b["status"]) and np.array_equal(step_a["material"], step_b["material"])
    assert np.array_equal(np.isfinite(step_a["t"]), hit)
    # values
    err_t = max(rel(got["t"][hit], want["t"][hit]), rel(step_a["t"][hit], step_b["t"][hit]))
    err_uv = np.abs(got["uv"][hit] - want["uv"][hit])
    uv_limit = uv_bound(want["normal"][hit]) if name in ("sphere", "moving sphere") else np.full((int(hit.sum()), 1), 1e-12)
    normal = forward_normals(want["normal"][hit], hit)
    err_n = float(np.abs(got["normal"][hit] - normal).max())
    unit = float(np.abs(np.sqrt(dot3(got["normal"][hit], got["normal"][hit])) - 1.0).max())
    scattered = (step_b["material"] == 0) & hit
    assert scattered.sum() > 500
    # The scattered ray starts at (L P') + t with P' = o' + t d', and t is the step's own: a ray that grazes a flat face has a t
    # that is ill-conditioned in the local ray (t = (D - n . o') / (n . d'), relative error eps |n| |d'| / |n . d'|, held to T_REL
    # above), and the reference's origin moved by that much along the ray is no statement about the way back.  So P' is restated
    # in numpy from the restated local ray and the step's t, and pushed forward by the restatement.
    local = tr.as_stored(ro[scattered] + tr.as_stored(step_a["t"][scattered][:, None] * rd[scattered]))
    P = forward_points(local, scattered)
    reach = step_a["t"][scattered] * np.sqrt(dot3(d[scattered], d[scattered]))
    limit_o = 64.0 * EPS * (np.sqrt(dot3(P, P)) + reach)
    err_o = np.abs(step_a["origin"][scattered] - P).max(axis=1)
    print(f"{label}: t {err_t:.3g} relative (bound {T_REL:.3g}), uv {err_uv.max():.3g} (share of its bound {float((err_uv / uv_limit).max()):.3g}), "
          f"normal {err_n:.3g} (bound {NORMAL_ABS:.3g}), | |n| - 1 | {unit:.3g}, origin {float((err_o / limit_o).max()):.3g} of its bound; "
          f"{out.sum()} of {n} rays left out")
    assert err_t <= T_REL
    assert np.all(err_uv <= uv_limit)
    assert err_n <= NORMAL_ABS and unit <= UNIT_ABS
    assert np.all(err_o <= limit_o)
    # the streams: the restatement of the rejection loop is the strict step's, and on the rays it keeps the fast step's as well
    assert np.array_equal(after, step_b["rng_state"]), "the restated loop is the strict build's"
    assert np.array_equal(step_a["rng_state"][keep], step_b["rng_state"][keep])
    return dict(t=err_t, uv=float(err_uv.max()), normal=err_n, left_out=out.mean())


def placed_case(name, chain_name):
    A, chain = tg.placed(name, chain_name)
    lo, ld, tm = tg.designed_local_rays(name, np.random.default_rng(28))
    o, d = tr.forward_points(chain, lo), tr.forward_vectors(chain, ld)
    ro, rd = tr.local_rays(chain, o, d)
    assert max(np.abs(ro - lo).max(), np.abs(rd - ld).max()) < 1e-12 * 40.0, "the restated local rays keep the designed margins"
    return A, chain, o, d, ro, rd, tm


def moved_case(name, chain_name):
    A, chain = mtg.moved(name, chain_name)
    lo, ld, tm = mtg.designed_rays_at_any_time(name, np.random.default_rng(32))
    o, d = mr.forward_points(chain, lo, tm), mr.forward_vectors(chain, ld, tm)
    ro, rd = mr.local_rays(chain, o, d, tm)
    assert max(np.abs(ro - lo).max(), np.abs(rd - ld).max()) < 4e-11, "the restated local rays keep the designed margins"
    return A, chain, o, d, ro, rd, tm


@pytest.mark.parametrize("chain_name", sorted(CHAINS))
@pytest.mark.parametrize("name", CHILDREN)
def test_a_placed_child_in_the_fast_build(name, chain_name):
    A, chain, o, d, ro, rd, tm = placed_case(name, chain_name)
    check_child(f"{name} under {chain_name}", name, A, tg.alone(name), o, d, ro, rd, tm,
                lambda p, rows: tr.forward_points(chain, p), lambda v, rows: tr.forward_normals(chain, v))


@pytest.mark.parametrize("chain_name", sorted(MOVING_CHAINS))
@pytest.mark.parametrize("name", CHILDREN)
def test_a_moved_child_in_the_fast_build(name, chain_name):
    A, chain, o, d, ro, rd, tm = moved_case(name, chain_name)
    assert ((tm < 0.0) | (tm > 1.0)).mean() >= 0.1, "times outside the keys: clamped"
    check_child(f"{name} under {chain_name}", name, A, tg.alone(name), o, d, ro, rd, tm,
                lambda p, rows: mr.forward_points(chain, p, tm[rows]), lambda v, rows: mr.forward_normals(chain, v, tm[rows]))


@pytest.mark.parametrize("moving", [False, True], ids=["placed", "moved"])
def test_the_fast_objects_are_the_ones_that_ran(moving):
    """Under the chain with shear, scale and rotation the fast t of some child differs in bits from the strict t of the same scene
    and rays -- a launcher that named the strict twin would give the same bits -- and both kernels report their registers."""
    differing, vgprs = {}, set()
    for name in CHILDREN:
        case = moved_case(name, "shear and scale between two rotations") if moving else placed_case(name, "shear scale rotation")
        A, o, d, tm = case[0], case[2], case[3], case[6]
        (fast, fst), (strict, sst) = (A.intersect(o, d, times=tm, seed=SEED, variant=v, want=("t",), stats=True) for v in (1, 0))
        (_, fstep), (_, sstep) = (A.path_step(o, d, times=tm, seed=SEED, variant=v, want=("t",), stats=True) for v in (1, 0))
        differing[name] = int(np.sum(bits(fast["t"]) != bits(strict["t"])))
        vgprs.add((fst.kernel_vgprs, sst.kernel_vgprs, fstep.kernel_vgprs, sstep.kernel_vgprs))
        assert min(fst.kernel_vgprs, sst.kernel_vgprs, fstep.kernel_vgprs, sstep.kernel_vgprs) > 0
    print(f"{'moved' if moving else 'placed'}: rays whose fast t differs in bits from the strict t: {differing}; "
          f"VGPRs (query fast, strict, step fast, strict): {sorted(vgprs)}")
    assert max(differing.values()) > 0


@pytest.mark.parametrize("scale", tg.ELLIPSOID_SCALES)
def test_the_analytic_ellipsoid_in_the_fast_build(scale):
    """tests/test_transform_gpu.py's closed form in long double, held to this file's bounds on t and the normal."""
    r = tg.ellipsoid_deviations(scale, variant=1)
    n = r["got"]["normal"]
    unit = float(np.abs(np.sqrt(dot3(n, n)) - 1.0).max())
    print(f"| |n| - 1 | {unit:.3g}")
    assert r["err_t"] <= T_REL and r["err_n"] <= NORMAL_ABS and unit <= UNIT_ABS, r["message"]


# ---- 2. routes and frames ----
def to_device(a):
    return torch.from_numpy(np.array(a)).cuda()


def as_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def builtin(scene_id, world_kind):
    return rt.sky_demo_scene(world_kind, W, H) if scene_id == 15 else rt.builtin_scene(scene_id, world_kind, W, H)


WORLDS = {}
for _name in sorted(tg.ROUTES):
    WORLDS[f"static {_name}"] = (lambda n=_name: (tg.route_scene(n), tg.route_rays(n)))
    WORLDS[f"moving {_name}"] = (lambda n=_name: (mtg.route_scene(n, None, (0.0, 1.0))[0], mtg.rays_of_shutter((0.0, 1.0), n in ("list world", "bvh world"))))
for _id in (13, 14, 15):
    for _kind in (0, 1):
        WORLDS[f"scene {_id} world {_kind}"] = (lambda i=_id, k=_kind: (lambda s: (s, camera_rays(s)))(builtin(i, k)))


def check_routes_and_frames(label, scene, rays, W=W, H=H, depth=50):
    """What section 2 asks of a world in the fast build; ``rays``: the camera rays of its 1-spp frame with their streams.  Returns
    the 4-spp fast frame, the fast ray query at the centre rays and the feature pass's albedo."""
    N = W * H
    o, d, tm, states = (np.array(a) for a in rays)
    # within the fast build, bit for bit: 3 + 5 accumulated samples are 8 at once
    eight, st8 = scene.render(W, H, 8, seed=SEED, max_depth=depth, variant=1)
    film = rt.Film(W, H)
    film.render(scene, 3, seed=SEED, max_depth=depth, variant=1, flags=ACCUMULATE)
    film.render(scene, 5, seed=SEED, max_depth=depth, variant=1, flags=ACCUMULATE | KEEP)
    assert np.array_equal(bits(film.download()), bits(eight))
    assert np.isfinite(eight).all() and eight.mean() > 0.02
    # ... and an adaptive film's pixel that stopped at n is the n-sample render's, as tests/test_adaptive_gpu.py holds both builds to
    film = rt.Film(W, H)
    film.set_adaptive(4, 2, 0.35)
    ast = film.render(scene, 8, seed=SEED, max_depth=depth, variant=1)
    counts, pixels = film.sample_counts(), film.download()
    assert ast.kernel_kind == st8.kernel_kind + tg.ADAPTIVE
    for c in np.unique(counts).tolist():
        plain = eight if c == 8 else scene.render(W, H, c, seed=SEED, max_depth=depth, variant=1)[0]
        assert np.array_equal(bits(pixels)[counts == c], bits(plain)[counts == c]), c
    # ... and the numpy and the torch call paths are one kernel
    record = ("t", "normal", "uv", "front_face", "material")
    host = scene.intersect(o, d, times=tm, seed=SEED, variant=1, want=record)
    dev = as_numpy(scene.intersect(to_device(o), to_device(d), times=to_device(tm), seed=SEED, variant=1, want=record))
    for key in record:
        assert np.array_equal(bits(host[key]), bits(dev[key])), key
    outputs = ("status", "emitted", "attenuation", "origin", "direction", "t", "rng_state")
    host_step = scene.path_step(o, d, times=tm, rng_state=states, variant=1, want=outputs)
    dev_step = as_numpy(scene.path_step(to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), variant=1, want=outputs))
    for key in outputs:
        assert np.array_equal(bits(host_step[key]), bits(dev_step[key])), key
    rad = {}
    for v in (0, 1):
        rad[v] = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=depth, variant=v, want=("radiance", "path_rays", "rng_state"))
    dev_rad = as_numpy(scene.radiance(to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), samples=1, max_depth=depth,
                                      variant=1, want=("radiance", "path_rays", "rng_state")))
    for key in dev_rad:
        assert np.array_equal(bits(rad[1][key]), bits(dev_rad[key])), key
    assert rad[1]["path_rays"].max() > 2
    # fast against strict: the frames, and the yardstick of the 1-spp frames for everything that follows single paths
    (one1, s1), (one0, s0) = (scene.render(W, H, 1, seed=SEED, max_depth=depth, variant=v) for v in (1, 0))
    (four1, f1), (four0, f0) = (scene.render(W, H, 4, seed=SEED, max_depth=depth, variant=v) for v in (1, 0))
    share = _share_that_differs(one0.reshape(N, 3), one1.reshape(N, 3))
    within1, within4 = compare(one1, one0)[1], compare(four1, four0)[1]
    assert s1.kernel_kind == s0.kernel_kind and f1.kernel_kind == f0.kernel_kind and s1.kernel_vgprs > 0
    ray_share = max(abs(int(s1.rays) - int(s0.rays)) / s0.rays, abs(int(f1.rays) - int(f0.rays)) / f0.rays)
    query = _share_that_differs(rad[0]["radiance"], rad[1]["radiance"])
    runs = {}
    for v in (0, 1):
        batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), variant=v)
        run = batch.run(depth)
        torch.cuda.synchronize()
        runs[v] = run.cpu().numpy()
    advance = _share_that_differs(runs[0], runs[1])
    print(f"{label}: kernel kind {s1.kernel_kind} ({s1.kernel_vgprs} VGPRs fast, {s0.kernel_vgprs} strict); within 1e-5 of the strict frame: "
          f"{within1:.4f} at 1 spp, {within4:.4f} at 4 spp; differ by more than 1e-9: {share * N:.0f} pixels, {query * N:.0f} radiance rays, "
          f"{advance * N:.0f} advanced rays of {N}; rays differ by {ray_share:.5f}")
    assert within1 >= WITHIN_FAST and within4 >= WITHIN_FAST
    assert ray_share <= share + EXTRA_SHARE
    assert query <= share + EXTRA_SHARE and advance <= share + EXTRA_SHARE
    # the feature pass at the centre rays against the fast ray query
    co, cd, time0, _ = centre_rays(scene, W, H)
    seen = scene.intersect(co, cd, times=np.full(N, time0), want=("t", "normal", "albedo"), seed=SEED, variant=1)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=SEED, variant=1)
    albedo, normal, distance = (p.reshape(N, -1) for p in film.features())
    assert np.array_equal(np.isfinite(seen["t"]), distance[:, 0] > 0)
    err_n, err_a = float(np.abs(seen["normal"] - normal).max()), float(np.abs(seen["albedo"] - albedo).max())
    print(f"{label}: feature pass against the ray query: normals {err_n:.3g}, albedo {err_a:.3g}")
    assert err_n <= 1e-12 and err_a <= 1e-12
    # the routes with light samples, where the world has a lamp: the same yardstick from the 1-spp frames with light samples
    if scene.info()["n_lights"]:
        frames = {}
        for v in (0, 1):
            direct = rt.Film(W, H)
            dst = direct.render(scene, 1, direct="mis", seed=SEED, max_depth=depth, variant=v)
            frames[v] = (direct.download().reshape(N, 3), dst.kernel_kind)
        share = _share_that_differs(frames[0][0], frames[1][0])
        mis = [scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=depth, variant=v, direct="mis")["radiance"] for v in (0, 1)]
        runs = []
        for v in (0, 1):
            batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states), variant=v, direct="mis")
            run = batch.run(depth)
            torch.cuda.synchronize()
            runs.append(run.cpu().numpy())
        within = compare(frames[1][0], frames[0][0])[1]
        query, advance = _share_that_differs(mis[0], mis[1]), _share_that_differs(runs[0], runs[1])
        print(f"{label}, with light samples: kernel kind {frames[1][1]}; within 1e-5 of the strict frame {within:.4f}; differ by more than 1e-9: "
              f"{share * N:.0f} pixels, {query * N:.0f} radiance rays, {advance * N:.0f} advanced rays of {N}")
        assert frames[1][1] == frames[0][1] and frames[1][1] & 1024 and within >= WITHIN_FAST
        assert query <= share + EXTRA_SHARE and advance <= share + EXTRA_SHARE
    return dict(frame=four1, stats=f1, seen=seen, albedo=albedo, centre_rays=(co, cd))


@pytest.mark.parametrize("label", sorted(WORLDS))
def test_routes_and_frames_in_the_fast_build(label):
    scene, rays = WORLDS[label]()
    check_routes_and_frames(label, scene, rays)


@pytest.mark.parametrize("tau", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("name", sorted(mtg.ROUTES))
def test_a_frozen_time_is_the_static_instance_in_the_fast_build(name, tau):
    (A, _), (B, _) = mtg.route_scene(name, None, (tau, tau)), mtg.route_scene(name, tau, (tau, tau))
    (fa, sa), (fb, sb) = (x.render(W, H, 4, seed=SEED, variant=1) for x in (A, B))
    exact, within, worst = compare(fa, fb)
    print(f"{name} at {tau}: kernel kind {sa.kernel_kind}; moving against static, both fast: bit-equal {exact:.4f}, within 1e-5 {within:.4f}, max |d| {worst:.3g}")
    assert sa.kernel_kind == sb.kernel_kind and within >= WITHIN_FAST and fa.mean() > 0.02


def test_a_sphere_under_a_moving_translate_is_the_moving_sphere_in_the_fast_build():
    c0, c1, radius = tg.MOVING
    scenes = []
    for build in (lambda s, grey: s.MovingTranslate(s.Sphere((0, 0, 0), radius, grey), c0, c1), lambda s, grey: s.MovingSphere(c0, c1, 0.0, 1.0, radius, grey)):
        s = rt.Scene()
        s.SetWorld(s.HittableList([build(s, s.Lambertian((0.5, 0.6, 0.7)))]))
        s.Camera((0.0, 0.0, 4.0), (0.4, -0.05, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 1.0)   # the sphere fills a third of the film
        s.Commit()
        scenes.append(s)
    a, b = scenes
    (fa, _), (fb, _) = (x.render(W, H, 4, seed=SEED, variant=1) for x in (a, b))
    exact, within, worst = compare(fa, fb)
    o, d, tm = tg.designed_local_rays("moving sphere", np.random.default_rng(33), count=1500)
    got, want = (x.intersect(o, d, times=tm, variant=1, want=("t", "normal", "front_face")) for x in (a, b))
    hit = np.isfinite(want["t"])
    err_t, err_n = np.abs(got["t"][hit] / want["t"][hit] - 1.0).max(), np.abs(got["normal"][hit] - want["normal"][hit]).max()
    on_film = float(np.mean(np.isfinite(b.intersect(*centre_rays(b, W, H)[:2], time=0.5, variant=1, want=("t",))["t"])))
    print(f"frames: bit-equal {exact:.4f}, within 1e-5 {within:.4f}, max |d| {worst:.3g}, the sphere covers {on_film:.3f} of the film; "
          f"designed rays: t {err_t:.3g} relative, normals {err_n:.3g}")
    assert within >= WITHIN_FAST and on_film > 0.05
    assert np.array_equal(np.isfinite(got["t"]), hit) and np.array_equal(hit, np.arange(len(o)) % 4 != 3)
    assert err_t <= T_REL and err_n <= NORMAL_ABS and np.array_equal(got["front_face"], want["front_face"])


@pytest.mark.parametrize("scene_id", [13, 14, 15])
def test_rtow_without_a_variant_renders_the_fast_frame(scene_id, tmp_path):
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    out, want = tmp_path / "rtow.ppm", tmp_path / "api.ppm"
    run = subprocess.run([exe, "--scene", str(scene_id), "--width", str(W), "--height", str(H), "--spp", "2", "--output", str(out)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    frame, st = builtin(scene_id, 0).render(W, H, 2, variant=1)
    strict, _ = builtin(scene_id, 0).render(W, H, 2, variant=0)
    rt.write_ppm(want, frame)
    print(f"scene {scene_id}: kernel kind {st.kernel_kind}, the fast frame differs in bits from the strict one on "
          f"{int(np.sum((bits(frame) != bits(strict)).any(axis=-1)))} of {N} pixels")
    assert out.read_bytes() == want.read_bytes()


@pytest.mark.parametrize("kind", ["quad", "triangle"])
def test_a_lamp_under_a_transform_in_the_fast_build(kind):
    """light and rng_state hold no contractable arithmetic; the direction to 1e-12; pdf = d^2 / (cos area) * chance within
    64 eps / cos relative, the bound of tests/test_lights_gpu.py."""
    s = tg.lamp_room(kind)
    L = s.lights()
    rng = np.random.default_rng(30)
    P = np.ascontiguousarray(np.stack([rng.uniform(-6, 6, 2000), np.full(2000, -1.0), rng.uniform(-6, 6, 2000)], axis=-1))
    nrm = np.ascontiguousarray(np.broadcast_to((0.0, 1.0, 0.0), P.shape))
    mat = np.zeros(len(P), dtype=np.uint8)
    states = lr.seeded_states(len(P), SEED)
    outputs = ("direction", "distance", "pdf", "light", "rng_state")
    for strategy in (0, 1):
        want = lr.sample_lights(L, P, states, strategy=strategy, normals=nrm, materials=mat)
        got, st = s.sample_lights(P, nrm, mat, None, states, strategy=strategy, variant=1, want=outputs, stats=True)
        valid = want["valid"]
        assert valid.mean() > 0.9 and st.kernel_vgprs > 0
        assert np.array_equal(got["light"], want["light"]) and np.array_equal(got["rng_state"], want["rng_state"])
        assert np.array_equal(got["pdf"] > 0.0, valid)
        cos = np.abs((L["n"][want["light"]] * want["direction"]).sum(axis=1))[valid]
        err_d = float(np.abs(got["direction"] - want["direction"]).max())
        err_p = np.abs(got["pdf"][valid] / want["pdf"][valid] - 1.0)
        print(f"{kind}, strategy {strategy}: direction {err_d:.3g}, pdf {err_p.max():.3g} relative ({float((err_p * cos / (64.0 * EPS)).max()):.3g} of its bound), "
              f"smallest cosine {cos.min():.3g}")
        assert err_d <= 1e-12 and np.all(err_p <= 64.0 * EPS / cos)
        # the density of the sampled direction asked for on its own, as tests/test_lights_gpu.py holds it to the sampled one
        out = s.light_pdf(np.ascontiguousarray(P[valid]), np.ascontiguousarray(got["direction"][valid]), None, strategy=strategy, variant=1,
                          want=("pdf", "light"))
        assert np.array_equal(out["light"], want["light"][valid])
        assert np.all(np.abs(out["pdf"] - got["pdf"][valid]) <= (64.0 * EPS / cos) * got["pdf"][valid])
