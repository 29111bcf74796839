"""Moving instances on the GPU (include/rtow.h rt_moving_transform): a child under moving chains answers a world ray of any time
as the child alone answers the restated local ray (tests/motion_restated.py), bit for bit in the strict build; with the shutter
frozen at one time every route and product is the static Transform's of that time; with the shutter open the frame is the
radiance along its camera rays and a list and a BvhNode world render the same bits although the children travel three times
their size; a Sphere under MovingTranslate is the MovingSphere.  Every ray set is a few thousand rays, every frame 32 x 24."""
import functools

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import light_restated as lr
import motion_restated as mr
import test_transform_gpu as tg
from query_helpers import bits, centre_rays, dot3, sphere_roots
from test_motion_transform_host import MOVING_CHAINS, washed
from test_path_step_gpu import fold
from test_radiance_gpu import camera_rays
from triangle_meshes import icosphere
from test_transform_gpu import ADAPTIVE, CHILDREN, N, RECORD, SEED, W, H, affine, rotation

pytestmark = pytest.mark.gpu


# ---- 5. restated from public calls, bit for bit ----
@functools.lru_cache(maxsize=None)
def moved(name, chain_name):
    s = rt.Scene()
    handle, chain = mr.build_chain(s, tg.child_of(s, name), MOVING_CHAINS[chain_name])
    return tg.committed(s, s.HittableList([handle])), chain


def designed_rays_at_any_time(name, rng):
    """tests/test_transform_gpu.py's designed local rays with ray times uniform in [-0.25, 1.25].  The MovingSphere child does not
    clamp: its rays are shifted with its centre from the time they were designed for to the time they carry."""
    lo, ld, designed_for = tg.designed_local_rays(name, rng)
    tm = np.ascontiguousarray(rng.uniform(-0.25, 1.25, len(lo)))
    if name == "moving sphere":
        lo = np.ascontiguousarray(lo + (tm - designed_for)[:, None] * (tg.MOVING[1] - tg.MOVING[0]))
    return lo, ld, tm


@pytest.mark.parametrize("chain_name", sorted(MOVING_CHAINS))
@pytest.mark.parametrize("name", CHILDREN)
def test_a_moved_child_answers_as_the_child_alone_answers_the_restated_local_ray(name, chain_name):
    A, chain = moved(name, chain_name)
    B = tg.alone(name)
    lo, ld, tm = designed_rays_at_any_time(name, np.random.default_rng(32))
    o = mr.forward_points(chain, lo, tm)
    d = mr.forward_vectors(chain, ld, tm)
    ro, rd = mr.local_rays(chain, o, d, tm)
    drift = max(np.abs(ro - lo).max(), np.abs(rd - ld).max())
    clamped = float(((tm < 0.0) | (tm > 1.0)).mean())
    print(f"{name} under {chain_name}: drift of the restated local rays {drift:.3g}, {clamped:.3f} of the times clamped")
    assert drift < 4e-11, drift   # the restated local rays keep the designed margins
    assert clamped >= 0.1
    kw = dict(times=tm, seed=SEED)
    got = A.intersect(o, d, want=RECORD + ("normal",), **kw)
    want = B.intersect(ro, rd, want=RECORD + ("normal",), **kw)
    hit = np.isfinite(want["t"])
    miss = np.arange(len(o)) % 4 == 3
    if name != "medium":
        assert hit[~miss].all() and not hit[miss].any(), "the aimed rays hit, the others miss"
    else:
        assert 0.3 < hit[~miss].mean() < 1.0 and not hit[miss].any(), "some rays scatter in the fog, some pass"
    for key in RECORD:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, int(np.sum(bits(got[key]) != bits(want[key]))))
    if name == "medium":
        assert np.array_equal(bits(got["normal"]), bits(want["normal"]))
    else:
        normal = mr.as_stored(0.0 + mr.forward_normals(chain, want["normal"][hit], tm[hit]))
        assert np.array_equal(bits(got["normal"][hit]), bits(normal)), int(np.sum((bits(got["normal"][hit]) != bits(normal)).any(axis=-1)))
        assert np.abs(np.sqrt(dot3(normal, normal)) - 1.0).max() < 1e-15 * 4
    states = lr.seeded_states(len(o), SEED)
    outputs = ("status", "t", "origin", "material", "rng_state")
    step_a = A.path_step(o, d, times=tm, rng_state=states, want=outputs)
    step_b = B.path_step(ro, rd, times=tm, rng_state=states, want=outputs)
    assert np.array_equal(step_a["status"], step_b["status"]) and np.array_equal(step_a["rng_state"], step_b["rng_state"])
    assert np.array_equal(bits(step_a["t"]), bits(step_b["t"])), "t is the world's t, through a medium as well"
    assert np.isfinite(step_b["t"]).sum() > 300
    if name != "medium":
        scattered = (step_b["material"] == 0) & hit
        assert scattered.sum() > 500
        P = mr.forward_points(chain, step_b["origin"][scattered], tm[scattered])
        assert np.array_equal(bits(step_a["origin"][scattered]), bits(P))


# ---- 6, 7. every route, with the shutter frozen and open ----
TURN_DEGREES = 12.0


def keys_of(m0, m1):
    """What rt_moving_transform stores for keys at times 0 and 1 (tests/test_motion_transform_host.py pins it to the bit)."""
    return m0[:, :3].copy(), m0[:, 3].copy(), m1[:, :3] - m0[:, :3], m1[:, 3] - m0[:, 3], 0.0, 1.0


def key_pair(m, travel, amount):
    """The two keys that stand for the static matrix ``m``: m itself and m turned and shifted by ``amount`` of TURN_DEGREES and ``travel``."""
    m0 = washed(m)
    turn = washed(rotation((0.2, 1.0, -0.3), TURN_DEGREES * amount))
    return m0, affine(washed(turn @ m0[:, :3]), m0[:, 3] + amount * np.asarray(travel, dtype=np.float64))


class Placer:
    """Stands where tests/test_transform_gpu.py calls Scene.Transform(child, m): ``tau`` None places a moving step from m to a
    turned and shifted m, a number places the static Transform of the matrix that a ray of that time sees."""

    def __init__(self, tau, amount):
        self.tau, self.amount = tau, amount   # amount: the share of TURN_DEGREES and of every travel that key 1 differs by

    def __call__(self, s, child, m, travel):
        m0, m1 = key_pair(m, travel, self.amount)
        if self.tau is None:
            return s.MovingTransform(child, m0, m1)
        return s.Transform(child, mr.frozen_matrix(keys_of(m0, m1), self.tau))


# from, at, vertical field of view.  The two worlds without media look along the travel of the third child, which fills much of the
# frame all the way; the others keep the room's camera.
CAMERAS = {True: ((1.3, 0.0, 30.0), (1.3, -0.85, 4.0), 9.0), False: ((0.0, 1.0, 14.0), (0.0, 0.5, 0.0), 45.0)}
TRAVEL = (0.0, 0.0, 11.8)   # of the three placed children in the two worlds without media: more than three times their size
SMALL = (0.2, 0.1, -0.1)    # (asserted below).  Where a medium stands in a BvhNode world the reference's walk meets it in the tree's
# order, and whether it draws depends on what was found before it (R/ConstantMedium.h clips to the caller's interval first): a frame
# is the static twin's only under the same tree, so there the keys differ by a 64th of that and the test asserts that the trees are equal.
# A list world has no such order: "object tree, list world" takes the full amount under the room's camera.
FULL = ("list world", "bvh world", "object tree, list world")


def place_chain(s, place, child, steps, travel):
    handle = child
    outermost = [k for k, (kind, _) in enumerate(steps) if kind == "transform"][0]
    for k in range(len(steps) - 1, -1, -1):
        kind, arg = steps[k]
        if kind == "translate":
            handle = s.Translate(handle, arg)
        elif kind == "rotate_y":
            handle = s.RotateY(handle, arg)
        else:
            handle = place(s, handle, arg, travel if k == outermost else SMALL)
    return handle


def fog_on_a_placed_box(s, place):
    box = place(s, s.MakeBox(tg.BOX_LO, tg.BOX_HI, s.Lambertian((1, 1, 1))), affine(rotation((0, 0, 1), 20.0) @ np.diag((2.0, 3.0, 2.0)), (3.0, 0.0, 1.0)), (-1.0, 0.5, 0.5))
    return [s.ConstantMedium(box, 0.6, (0.9, 0.9, 0.9))]


def many_boxes_and_fog(s, place, marble=False):
    grey = s.Lambertian(s.NoiseTexture(4.0, rt.Rng(SEED, 0))) if marble else s.Lambertian((0.4, 0.4, 0.6))
    boxes = [s.MakeBox((-5.5 + 0.9 * (k % 12), -4.0, 2.0 + 0.9 * (k // 12)), (-4.8 + 0.9 * (k % 12), -3.6 + 0.05 * (k % 5), 2.7 + 0.9 * (k // 12)), grey)
             for k in range(36)]
    return boxes + fog_on_a_placed_box(s, place)


def placed_fog(s, place):
    fog = s.ConstantMedium(s.MakeBox(tg.BOX_LO, tg.BOX_HI, s.Lambertian((1, 1, 1))), 1.5, (0.9, 0.9, 0.9))
    return [place(s, fog, affine(rotation((1, 0, 0), -25.0) @ np.diag((2.5, 2.0, 2.0)), (3.0, 0.5, 1.0)), (-1.5, 0.5, 0.0))]


ROUTES = {   # tests/test_transform_gpu.py's six, every Transform step placed by a Placer
    "list world": (lambda s, p: [], "list"),
    "bvh world": (lambda s, p: [], "bvh"),
    "bvh world with a fog": (many_boxes_and_fog, "bvh"),
    "general kernel with a fog": (lambda s, p: many_boxes_and_fog(s, p, True), "bvh"),
    "object tree": (placed_fog, "bvh"),
    "object tree, list world": (placed_fog, "list"),
}
PLACED = (("box", "shear scale rotation"), ("sphere", "mirror"), ("icosahedron", "translate transform rotate_y transform"))


@functools.lru_cache(maxsize=None)
def route_scene(name, tau, shutter):
    """tests/test_transform_gpu.py's room.  Returns (scene, the handles of the three placed children)."""
    extra, world = ROUTES[name]
    wide = name in ("list world", "bvh world")
    s, place = rt.Scene(), Placer(tau, 1.0 if name in FULL else 1.0 / 64.0)
    white, light = s.Lambertian((0.73, 0.73, 0.73)), s.DiffuseLight((7.0, 7.0, 7.0))
    items = [s.Quad((-6, -4, -6), (12, 0, 0), (0, 0, 12), white), s.Quad((-6, 6, -6), (12, 0, 0), (0, 0, 12), white),
             s.Quad((-6, -4, -6), (12, 0, 0), (0, 10, 0), s.Lambertian((0.12, 0.45, 0.15))),
             s.Quad((-2, 5.9, -2), (4, 0, 0), (0, 0, 4), light)]
    children = []
    for k, (child, chain_name) in enumerate(PLACED):
        steps = [("translate", (-3.5 + 1.5 * k, -1.0, -2.0 + 0.5 * k))] + tg.CHAINS[chain_name]
        children.append(place_chain(s, place, tg.child_of(s, child), steps, TRAVEL))
    items += children + extra(s, place)
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera(CAMERAS[wide][0], CAMERAS[wide][1], (0, 1, 0), CAMERAS[wide][2], W / H, 0.0, 1.0, shutter[0], shutter[1], (0.1, 0.1, 0.15))
    s.Commit()
    return s, tuple(children)


@functools.lru_cache(maxsize=None)
def rays_of_shutter(shutter, wide):
    arrays = camera_rays(route_scene("list world" if wide else "object tree", None, shutter)[0])   # one camera for the wide routes, one for the others
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.mark.parametrize("tau", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_a_frozen_time_is_the_static_instance(name, tau):
    (A, _), (B, _) = route_scene(name, None, (tau, tau)), route_scene(name, tau, (tau, tau))
    o, d, tm, states = rays_of_shutter((tau, tau), name in ("list world", "bvh world"))
    assert (tm == tau).all()
    if name not in FULL:
        assert np.array_equal(A.dump_nodes()[1], B.dump_nodes()[1]), "the premise where media stand in a tree: one tree on both sides"
    kinds = []
    for flags in (0, rt.FLAG_FORCE_GENERAL):
        (fa, sa), (fb, sb) = (x.render(W, H, 4, seed=SEED, variant=0, flags=flags) for x in (A, B))
        assert np.array_equal(bits(fa), bits(fb)), (flags, int(np.sum(bits(fa) != bits(fb))))
        kinds.append((sa.kernel_kind, sb.kernel_kind))
    print(f"{name} at {tau}: kernel kinds (moving, static) {kinds}")
    assert kinds[0][0] == kinds[0][1] and kinds[1][0] == kinds[1][1], "the routes' kernels are the static routes'"
    outputs = ("radiance", "path_rays", "rng_state")
    ra, rb = (x.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=0, want=outputs) for x in (A, B))
    for key in outputs:
        assert np.array_equal(bits(ra[key]), bits(rb[key])), key
    assert ra["path_rays"].max() > 2
    (acc_a, steps_a, final_a), (acc_b, steps_b, final_b) = (fold(x, o, d, tm, states, 50, {"status": set(), "material": set()}) for x in (A, B))
    assert np.array_equal(bits(acc_a), bits(acc_b)) and np.array_equal(steps_a, steps_b) and np.array_equal(final_a, final_b)
    assert np.array_equal(bits(acc_a), bits(ra["radiance"]))
    to_device = lambda a: torch.from_numpy(np.array(a)).cuda()
    runs = []
    for x in (A, B):
        batch = rt.PathBatch(x, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states))
        got = batch.run(50)
        torch.cuda.synchronize()
        runs.append(got.cpu().numpy())
    assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(ra["radiance"]))
    films = []
    for x in (A, B):
        film = rt.Film(W, H)
        film.set_adaptive(4, 2, 0.35)
        ast = film.render(x, 8, seed=SEED, variant=0)
        assert ast.kernel_kind & ADAPTIVE
        films.append((film.sample_counts(), film.download()))
    assert np.array_equal(films[0][0], films[1][0]) and np.array_equal(bits(films[0][1]), bits(films[1][1]))
    ma, mb = (x.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=8, variant=0, direct="mis")["radiance"] for x in (A, B))
    assert np.array_equal(bits(ma), bits(mb))


def restated_chain(k):
    """The chain of the k-th placed child of the full routes as tests/motion_restated.py takes it."""
    steps = [("translate", (-3.5 + 1.5 * k, -1.0, -2.0 + 0.5 * k))] + tg.CHAINS[PLACED[k][1]]
    outermost = [j for j, (kind, _) in enumerate(steps) if kind == "transform"][0]
    return [("moving", keys_of(*key_pair(arg, TRAVEL if j == outermost else SMALL, 1.0))) if kind == "transform" else (kind, arg)
            for j, (kind, arg) in enumerate(steps)]


def local_hit(name, o, d, tmin=0.001):
    """The smallest t > tmin at which the local rays meet the child of tests/test_transform_gpu.py, inf for a miss: numpy, on the CPU."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "sphere":
            near, far, _ = sphere_roots(o, d, tg.SPHERE_C, tg.SPHERE_R)
            cands = [near, far]
        elif name == "box":
            t0, t1 = (tg.BOX_LO - o) / d, (tg.BOX_HI - o) / d
            enter, leave = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
            cands = [np.where(enter <= leave, enter, np.nan), np.where(enter <= leave, leave, np.nan)]
        else:
            verts, faces = icosphere(0, tg.ICO_R)
            cands = []
            for a, b, c in faces:   # Moeller-Trumbore
                e1, e2 = verts[b] - verts[a], verts[c] - verts[a]
                pv = np.cross(d, e2)
                det = pv @ e1
                tv = o - verts[a]
                u = dot3(tv, pv) / det
                qv = np.cross(tv, e1)
                v = dot3(d, qv) / det
                cands.append(np.where((u >= 0) & (v >= 0) & (u + v <= 1), (qv @ e2) / det, np.nan))
        t = np.stack(cands)
        t = np.where(t > tmin, t, np.inf)
    return t.min(axis=0)


def key_boxes(name):
    """The boxes of the three placed children at the two keys, from the static twins: (3, 2, 3, 2)."""
    out = []
    for tau in (0.0, 1.0):
        s, children = route_scene(name, tau, (0.0, 1.0))
        out.append([np.array(s.BoundingBox(h)).reshape(3, 2) for h in children])
    return np.array(out).transpose(1, 0, 2, 3)


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_with_the_shutter_open_the_frame_is_the_radiance_along_its_camera_rays(name):
    scene, children = route_scene(name, None, (0.0, 1.0))
    o, d, tm, states = rays_of_shutter((0.0, 1.0), name in ("list world", "bvh world"))
    assert 0.0 <= tm.min() < 0.05 and 0.95 < tm.max() <= 1.0
    one, st = scene.render(W, H, 1, seed=SEED, variant=0)
    want = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=0, want=("radiance", "path_rays"))
    assert np.array_equal(bits(np.sqrt(want["radiance"])), bits(one.reshape(N, 3)))
    general, _ = scene.render(W, H, 1, seed=SEED, variant=0, flags=rt.FLAG_FORCE_GENERAL)
    assert np.array_equal(bits(one), bits(general))
    # the feature pass traces the centre rays at the camera's time0
    co, cd, time0, _ = centre_rays(scene, W, H)
    query = scene.intersect(co, cd, times=np.full(N, time0), want=("t", "normal", "albedo", "material"), seed=SEED)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=SEED, variant=0)
    albedo, normal, depth = (p.reshape(N, -1) for p in film.features())
    assert np.array_equal(np.isfinite(query["t"]), depth[:, 0] > 0)
    assert np.array_equal(bits(query["normal"]), bits(normal)) and np.array_equal(bits(query["albedo"]), bits(albedo))


def test_a_list_and_a_bvh_world_render_the_same_bits_while_the_children_travel():
    """What an endpoint-only or too-tight box would break: the children travel at least three times their own size during the
    shutter, and many camera rays meet them where neither key's box is."""
    (L, children), (Bv, _) = route_scene("list world", None, (0.0, 1.0)), route_scene("bvh world", None, (0.0, 1.0))
    for spp in (1, 4):
        (fl, _), (fb, _) = (x.render(W, H, spp, seed=SEED, variant=0) for x in (L, Bv))
        assert np.array_equal(bits(fl), bits(fb)), spp
    boxes = key_boxes("list world")
    for k in range(3):
        size = (boxes[k, 0, :, 1] - boxes[k, 0, :, 0]).max()
        travel = np.linalg.norm(boxes[k, 1].mean(axis=1) - boxes[k, 0].mean(axis=1))
        print(f"child {k}: size {size:.3f}, travel {travel:.3f}")
        assert travel >= 3.0 * size
    # The camera rays that hit a moving child at a position that neither key's box contains, on the CPU from the restatement: the
    # local ray of each child's chain at the ray's time, the child's own shape in plain float64 (no bits are compared here), the
    # nearest child, its hit point forward again; the boxes are the static twins' (BoundingBox of Transform(child, [L(s) | t(s)])).
    o, d, tm, _ = rays_of_shutter((0.0, 1.0), True)
    nearest, which, where = np.full(N, np.inf), np.full(N, -1), np.zeros((N, 3))
    for k in range(3):
        chain = restated_chain(k)
        lo, ld = mr.local_rays(chain, o, d, tm)
        t = local_hit(PLACED[k][0], lo, ld)
        P = mr.forward_points(chain, lo + np.where(np.isfinite(t), t, 0.0)[:, None] * ld, tm)
        closer = t < nearest
        nearest[closer], which[closer], where[closer] = t[closer], k, P[closer]
    between = np.zeros(N, dtype=bool)
    for k in range(3):
        inside = [((where >= boxes[k, e, :, 0]) & (where <= boxes[k, e, :, 1])).all(axis=1) for e in (0, 1)]
        between |= (which == k) & ~inside[0] & ~inside[1]
    print(f"{between.mean():.3f} of the camera rays hit a moving child where neither key's box is")
    assert between.mean() >= 0.05
    # ... and both worlds find those hits: the leaves are the items' positions in the list (a ray that grazes an edge may round otherwise)
    hitL, hitB = (x.intersect(o, d, times=tm, want=("t", "leaf")) for x in (L, Bv))
    assert np.array_equal(bits(hitL["t"]), bits(hitB["t"]))
    found = np.isfinite(hitL["t"][between]) & (hitL["leaf"][between] == 4 + which[between])
    assert found.mean() > 0.98 and np.abs(hitL["t"][between][found] / nearest[between][found] - 1.0).max() < 1e-9


# ---- 8. closed forms ----
def test_a_sphere_under_a_moving_translate_is_the_moving_sphere():
    c0, c1, radius = tg.MOVING
    a, b = rt.Scene(), rt.Scene()
    grey = a.Lambertian((0.5, 0.6, 0.7))
    tg.committed(a, a.HittableList([a.MovingTranslate(a.Sphere((0, 0, 0), radius, grey), c0, c1)]))
    tg.committed(b, b.HittableList([b.MovingSphere(c0, c1, 0.0, 1.0, radius, b.Lambertian((0.5, 0.6, 0.7)))]))
    o, d, tm = tg.designed_local_rays("moving sphere", np.random.default_rng(33), count=4000)   # times in [0, 1]: the sphere does not clamp
    got, want = (x.intersect(o, d, times=tm, want=("t", "normal", "front_face")) for x in (a, b))
    hit = np.isfinite(want["t"])
    miss = np.arange(len(o)) % 4 == 3
    assert np.array_equal(hit, ~miss) and np.array_equal(np.isfinite(got["t"]), hit), "the same rays hit"
    err_t = np.abs(got["t"][hit] / want["t"][hit] - 1.0).max()
    err_n = np.abs(got["normal"][hit] - want["normal"][hit]).max()
    print(f"t agrees to {err_t:.3g} relative, the normals to {err_n:.3g}")
    assert err_t <= 1e-12 and err_n <= 1e-12 and np.array_equal(got["front_face"], want["front_face"])


@pytest.mark.parametrize("name", CHILDREN)
def test_equal_keys_are_the_static_transform_bit_for_bit(name):
    m = affine(washed(rotation((1, 2, -0.5), 37.0) @ np.diag((1.7, 0.6, 1.2)) @ tg.SHEAR), (3.0, -1.5, 0.75))
    a, b = rt.Scene(), rt.Scene()
    ha = a.MovingTransform(tg.child_of(a, name), m, m, 0.25, 0.5)
    hb = b.Transform(tg.child_of(b, name), m)
    tg.committed(a, a.HittableList([ha]))
    tg.committed(b, b.HittableList([hb]))
    lo, ld, tm = designed_rays_at_any_time(name, np.random.default_rng(34))
    chain = [("transform", b.transform_matrices(hb))]
    o, d = mr.forward_points(chain, lo, tm), mr.forward_vectors(chain, ld, tm)
    outputs = RECORD + ("normal", "leaf", "albedo")
    got, want = (x.intersect(o, d, times=tm, seed=SEED, want=outputs) for x in (a, b))
    assert np.isfinite(want["t"]).mean() > 0.2
    for key in outputs:
        assert np.array_equal(bits(got[key]), bits(want[key])), key
