"""General affine instances on the GPU (include/rtow.h rt_transform): a child under a chain of Transforms answers a world ray as
the child alone answers the restated local ray (tests/transform_restated.py), bit for bit in the strict build; a scaled, turned
and moved unit sphere is the analytic ellipsoid; every route through the kernels and every product of the library sees the one
hit record; lamps under a Transform are sampled as the restatement samples the dumped rows; scene 14 renders.  Every ray set is
a few thousand rays, every frame at most 32 x 24 pixels."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import light_restated as lr
import transform_restated as tr
from query_helpers import bits, centre_rays, dot3
from test_path_step_gpu import fold
from test_radiance_gpu import camera_rays
from triangle_meshes import icosphere

pytestmark = pytest.mark.gpu

W, H = 32, 24
N = W * H
SEED = 1984
ADAPTIVE = 512   # rt_render_stats.kernel_kind


# ---- 1. restated from public calls, bit for bit ----
def rotation(axis, degrees):
    a, (x, y, z) = np.radians(degrees), np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def affine(L, t):
    return np.concatenate([np.asarray(L, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


SHEAR = np.array([[1.0, 0.35, -0.2], [0.0, 1.0, 0.15], [0.0, 0.0, 1.0]])
CHAINS = {
    "shear scale rotation": [("transform", affine(rotation((1, 2, -0.5), 37.0) @ np.diag((1.7, 0.6, 1.2)) @ SHEAR, (3.0, -1.5, 0.75)))],
    "mirror": [("transform", affine(np.diag((-1.3, 0.9, 1.1)), (-2.0, 0.5, 1.0)))],
    "translate transform rotate_y transform": [("translate", (1.25, -0.5, 2.0)),
                                               ("transform", affine(rotation((0.3, -1, 0.2), -63.0) @ np.diag((0.8, 1.4, 1.1)), (0.5, 0.25, -1.0))),
                                               ("rotate_y", 28.0),
                                               ("transform", affine(SHEAR.T @ np.diag((1.2, 0.9, -0.7)), (-0.3, 0.2, 0.1)))],
}
BOX_LO, BOX_HI = np.array((-0.5, -0.4, -0.6)), np.array((0.7, 0.5, 0.4))
SPHERE_C, SPHERE_R = np.array((0.3, -0.2, 0.1)), 0.8
MOVING = (np.array((0.3, -0.2, 0.1)), np.array((0.5, 0.1, -0.1)), 0.6)
ICO_R = 0.9


def child_of(s, name):
    grey = s.Lambertian((0.5, 0.6, 0.7))
    if name == "sphere":
        return s.Sphere(SPHERE_C, SPHERE_R, grey)
    if name == "moving sphere":
        return s.MovingSphere(MOVING[0], MOVING[1], 0.0, 1.0, MOVING[2], grey)
    if name == "box":
        return s.MakeBox(BOX_LO, BOX_HI, grey)
    if name == "icosahedron":
        verts, faces = icosphere(0, ICO_R)
        tex = np.stack([0.5 + 0.4 * verts[:, 0] / ICO_R, 0.5 + 0.4 * verts[:, 1] / ICO_R], axis=-1)
        return s.TriangleMesh(verts, faces, grey, normals=verts / ICO_R, texcoords=tex)
    assert name == "medium"
    return s.ConstantMedium(s.MakeBox(BOX_LO, BOX_HI, grey), 2.0, (0.8, 0.8, 0.8))


CHILDREN = ("sphere", "moving sphere", "box", "icosahedron", "medium")


def face_targets(rng, corners, per_face):
    """Points strictly inside triangles given as (Q, Q + u, Q + v): every barycentric coordinate >= 0.05."""
    out = []
    for q, a, b in corners:
        al, be = rng.uniform(0.05, 0.9, 3 * per_face), rng.uniform(0.05, 0.9, 3 * per_face)
        keep = al + be <= 0.95
        out.append((q + al[keep, None] * (a - q) + be[keep, None] * (b - q))[:per_face])
    out = np.concatenate(out)
    return out[rng.permutation(len(out))]


def box_faces(lo, hi):
    faces = []
    for axis in range(3):
        p, q = (axis + 1) % 3, (axis + 2) % 3
        for end in (lo, hi):
            c = lo.copy()
            c[axis] = end[axis]
            u, v = np.zeros(3), np.zeros(3)
            u[p], v[q] = hi[p] - lo[p], hi[q] - lo[q]
            faces += [(c, c + u, c + v), (c + u + v, c + v, c + u)]   # both triangles of the rectangle
    return faces


def designed_local_rays(name, rng, count=1500):
    """Local rays at the child with the margins the issue asks for -- face points with barycentric margin >= 0.05, sphere points at
    least 5 degrees inside the silhouette -- and a third as many that miss by far.  Returns (o, d, times)."""
    times = rng.uniform(0.0, 1.0, count)
    if name in ("sphere", "moving sphere"):
        if name == "sphere":
            centre, radius = np.broadcast_to(SPHERE_C, (count, 3)), SPHERE_R
        else:
            centre, radius = MOVING[0] + times[:, None] * (MOVING[1] - MOVING[0]), MOVING[2]
        n = rng.normal(size=(count, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        target = centre + radius * n
        # the origin on the normal's side, within 60 degrees of it: the hit is >= 30 degrees inside the silhouette as seen from afar,
        # and at the distance of 4 radii still more than 5 degrees
        side = rng.normal(size=(count, 3))
        side -= dot3(side, n)[:, None] * n
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        tilt = np.radians(rng.uniform(0.0, 60.0, count))[:, None]
        origin = target + 4.0 * radius * (np.cos(tilt) * n + np.sin(tilt) * side)
    else:
        if name == "icosahedron":
            verts, faces = icosphere(0, ICO_R)
            corners = [(verts[a], verts[b], verts[c]) for a, b, c in faces]
            centre, reach = np.zeros(3), ICO_R
        else:
            corners = box_faces(BOX_LO, BOX_HI)
            centre, reach = 0.5 * (BOX_LO + BOX_HI), 1.0
        target = face_targets(rng, corners, 2 * count // len(corners))[:count]
        assert len(target) == count
        # origins on a sphere about the child -- a convex body, so the aimed point is where the ray enters -- and every fourth one near
        # its centre, so that the aimed point is where it leaves, from behind the face
        n = rng.normal(size=(count, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        outward = target - centre
        n = np.where((dot3(n, outward) < 0.0)[:, None], -n, n)   # on the aimed face's side
        origin = np.where((np.arange(count) % 4 == 2)[:, None], centre + 0.1 * reach * n, centre + 4.0 * reach * n)
    d = (target - origin) * rng.uniform(0.5, 2.0, count)[:, None]   # (not unit vectors)
    miss = np.arange(count) % 4 == 3
    axis = np.eye(3)[np.argmin(np.abs(d[miss]), axis=1)]   # the misses leave at a right angle to the aimed direction
    d[miss] = np.cross(d[miss], axis)
    return np.ascontiguousarray(origin), np.ascontiguousarray(d), np.ascontiguousarray(times)


def committed(s, world):
    s.SetWorld(world)
    s.Camera((0.0, 0.0, 12.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 1.0)
    s.Commit()
    return s


@functools.lru_cache(maxsize=None)
def alone(name):
    s = rt.Scene()
    return committed(s, s.HittableList([child_of(s, name)]))


@functools.lru_cache(maxsize=None)
def placed(name, chain_name):
    s = rt.Scene()
    handle, chain = tr.build_chain(s, child_of(s, name), CHAINS[chain_name])
    return committed(s, s.HittableList([handle])), chain


RECORD = ("t", "front_face", "uv", "material")


@pytest.mark.parametrize("chain_name", sorted(CHAINS))
@pytest.mark.parametrize("name", CHILDREN)
def test_a_placed_child_answers_as_the_child_alone_answers_the_restated_local_ray(name, chain_name):
    A, chain = placed(name, chain_name)
    B = alone(name)
    lo, ld, tm = designed_local_rays(name, np.random.default_rng(28))
    o = tr.forward_points(chain, lo)
    d = tr.forward_vectors(chain, ld)
    ro, rd = tr.local_rays(chain, o, d)
    # the restated local rays are the designed ones up to rounding, so they keep the designed margins (checked here, on the CPU)
    drift = max(np.abs(ro - lo).max(), np.abs(rd - ld).max())
    assert drift < 1e-12 * 40.0, drift
    kw = dict(times=tm, seed=SEED)   # (the medium's test draws: both sides seeded alike)
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
    if name == "medium":   # (a medium's hit has no normal to speak of: the ray query reports zeros)
        assert np.array_equal(bits(got["normal"]), bits(want["normal"]))
    else:
        # the ray query stores 0 + n: no negative zeros on either side (a zero of Li may be one)
        normal = tr.as_stored(0.0 + tr.forward_normals(chain, want["normal"][hit]))
        assert np.array_equal(bits(got["normal"][hit]), bits(normal)), int(np.sum((bits(got["normal"][hit]) != bits(normal)).any(axis=-1)))
        assert np.abs(np.sqrt(dot3(normal, normal)) - 1.0).max() < 1e-15 * 4
        assert set(np.unique(want["front_face"][hit]).tolist()) == ({0, 1} if name in ("box", "icosahedron") else {1})
    # one bounce: the scattered ray starts at (L P') + t; the streams, and with them a medium's decision, are the child's
    states = lr.seeded_states(len(o), SEED)
    step_a = A.path_step(o, d, times=tm, rng_state=states, want=("status", "t", "origin", "material", "rng_state"))
    step_b = B.path_step(ro, rd, times=tm, rng_state=states, want=("status", "t", "origin", "material", "rng_state"))
    assert np.array_equal(step_a["status"], step_b["status"]) and np.array_equal(step_a["rng_state"], step_b["rng_state"])
    assert np.array_equal(bits(step_a["t"]), bits(step_b["t"])), "t is the world's t, through a medium as well"
    assert np.isfinite(step_b["t"]).sum() > 300
    scattered = (step_b["material"] == 0) & hit if name != "medium" else np.zeros(len(o), dtype=bool)
    if name != "medium":
        assert scattered.sum() > 500
        P = tr.forward_points(chain, step_b["origin"][scattered])
        assert np.array_equal(bits(step_a["origin"][scattered]), bits(P))


# ---- 2. against closed forms ----
ELLIPSOID_SCALES = [(1.5, 0.7, 1.1), (0.4, 2.5, 1.0)]


def ellipsoid_deviations(scale, variant=0):
    """The ellipsoid {x : |S^-1 R^T (x - c)| = 1} in extended precision against the library.  The bound, u = 2^-53: each of the two
    matrix steps forms a component of the local ray with 3 products, 2 sums and a subtraction from entries of Li that are good
    to 2 u cond, so o' and d' carry at most 8 u cond(L) relative to their length; a, b, c are bilinear in them (twice that)
    plus 4 u of their own: delta = 20 u cond(L).  With m = disc / b^2 (computed below for these rays, not assumed: m >= the
    margin, and m <= 0.1 from this distance), sqrt(disc) = |b| sqrt(m) has the absolute error delta |b| / sqrt(m) (disc = b^2 -
    a c loses 2 delta / m relatively, the root halves it), so the numerator -b - sqrt(disc), which is at least |b| (1 - sqrt(0.1)) =
    0.68 |b|, is good to delta (1 + 1 / sqrt(margin)) / 0.68, and the division by a adds delta:
        |dt| / t <= 20 u cond(L) (1 + 1.5 (1 + 1 / sqrt(margin))) < 24 u cond(L) (1 + 1 / sqrt(margin)) x 1.5
    The unit normal is Li^T applied to P' = o' + t d', known to |dt| / t times |t d'| / |P'| <= 6 (P' is a unit vector, t |d'| at most
    the distance 5 plus 1), and renormalised; Li^T amplifies a relative error by at most cond(L): 6 cond(L) times the bound on t.
    Returns what the library's ``variant`` build answers and how far it is from the closed form, for the tests to hold to a bound."""
    R = rotation((0.2, 0.4, 1.0), 33.0)
    centre = np.array((1.0, -2.0, 0.5))
    s = rt.Scene()
    ball = s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))
    handle, chain = tr.build_chain(s, ball, [("translate", centre), ("transform", affine(R, (0, 0, 0))), ("transform", affine(np.diag(scale), (0, 0, 0)))])
    committed(s, s.HittableList([handle]))
    rng = np.random.default_rng(29)
    n = rng.normal(size=(4000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    side = rng.normal(size=n.shape)
    side -= dot3(side, n)[:, None] * n
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    tilt = np.radians(rng.uniform(0.0, 60.0, len(n)))[:, None]
    lo = n + 4.0 * (np.cos(tilt) * n + np.sin(tilt) * side)   # local: aimed at the unit sphere's point n
    ld = (n - lo) * rng.uniform(0.5, 2.0, len(n))[:, None]
    L = R @ np.diag(scale)
    o = np.ascontiguousarray(lo @ L.T + centre)
    d = np.ascontiguousarray(ld @ L.T)
    got = s.intersect(o, d, variant=variant, want=("t", "normal", "front_face"))
    # the closed form, in long double from the exact inputs (R, scale, centre as float64 numbers)
    E = np.longdouble
    A = np.diag(1.0 / np.asarray(scale, dtype=E)) @ np.linalg.inv(R.astype(np.float64)).astype(E)   # refined below
    Lq = R.astype(E) @ np.diag(np.asarray(scale, dtype=E))
    for _ in range(3):   # Newton on the inverse, in long double: A <- A (2 I - Lq A)
        A = A @ (2.0 * np.eye(3, dtype=E) - Lq @ A)
    oq, dq = (o.astype(E) - centre.astype(E)) @ A.T, d.astype(E) @ A.T
    a, b, c = dot3(dq, dq), dot3(oq, dq), dot3(oq, oq) - 1.0
    disc = b * b - a * c
    margin = float((disc / (b * b)).min())
    t = (-b - np.sqrt(disc)) / a
    p = oq + t[:, None] * dq
    m = p @ A   # A^T p
    normal = m / np.sqrt(dot3(m, m))[:, None]
    cond = float(np.linalg.cond(L))
    u = 2.0 ** -53
    bound_t = 36.0 * u * cond * (1.0 + 1.0 / np.sqrt(margin))
    bound_n = 6.0 * cond * bound_t
    err_t = float(np.abs((got["t"].astype(E) - t) / t).max())
    err_n = float(np.abs(got["normal"].astype(E) - normal).max())
    message = (f"scale {scale}, variant {variant}: cond(L) {cond:.3f}, margin disc / b^2 >= {margin:.4f}; t: bound {bound_t:.3g}, largest deviation {err_t:.3g}; "
               f"normal: bound {bound_n:.3g}, largest deviation {err_n:.3g}")
    print(message)
    assert margin > np.sin(np.radians(5.0)) ** 2 and float((disc / (b * b)).max()) <= 0.1, message
    assert np.isfinite(got["t"]).all() and (got["front_face"] == 1).all(), message
    return dict(got=got, err_t=err_t, err_n=err_n, bound_t=bound_t, bound_n=bound_n, message=message)


@pytest.mark.parametrize("scale", ELLIPSOID_SCALES)
def test_a_scaled_turned_and_moved_unit_sphere_is_the_analytic_ellipsoid(scale):
    """ellipsoid_deviations has the closed form and derives the two bounds."""
    r = ellipsoid_deviations(scale)
    assert r["err_t"] <= r["bound_t"] and r["err_n"] <= r["bound_n"], r["message"]


def test_a_fog_is_measured_where_the_header_says():
    """The media rule against scenes that hold no Transform, with scales that are powers of two, so that the local ray, the box's
    planes and every t are the same bits on both sides and only the length the fog is measured along can differ.
    A ConstantMedium whose BOUNDARY is a Transform measures in the caller's space: a fog over Scale(box, (2, 4, 1/2)) is the fog of
    that density over the box built with the scaled corners.  A ConstantMedium UNDER a Transform measures in object space: a fog
    scaled by 2 is as opaque across its width as before, that is, the fog of half the density over the box of twice the size."""
    scale, density = np.array((2.0, 4.0, 0.5)), 0.75
    rng = np.random.default_rng(31)
    n = 3000
    target = rng.uniform(BOX_LO, BOX_HI, size=(n, 3))

    def rays(factor):
        aim = target * factor
        origin = aim + 6.0 * rng.normal(size=(n, 3))
        return np.ascontiguousarray(origin), np.ascontiguousarray((aim - origin) * rng.uniform(0.5, 2.0, n)[:, None])

    def fog_scene(build):
        s = rt.Scene()
        return committed(s, s.HittableList([build(s, s.Lambertian((1, 1, 1)))]))

    states = lr.seeded_states(n, SEED)
    want = ("status", "t", "origin", "rng_state")
    cases = [("boundary", scale,
              lambda s, m: s.ConstantMedium(s.Scale(s.MakeBox(BOX_LO, BOX_HI, m), scale), density, (0.8, 0.8, 0.8)),
              lambda s, m: s.ConstantMedium(s.MakeBox(BOX_LO * scale, BOX_HI * scale, m), density, (0.8, 0.8, 0.8))),
             ("under", np.array((2.0, 2.0, 2.0)),
              lambda s, m: s.Scale(s.ConstantMedium(s.MakeBox(BOX_LO, BOX_HI, m), density, (0.8, 0.8, 0.8)), 2.0),
              lambda s, m: s.ConstantMedium(s.MakeBox(BOX_LO * 2.0, BOX_HI * 2.0, m), density / 2.0, (0.8, 0.8, 0.8)))]
    for name, factor, placed_fog_, plain_fog in cases:
        o, d = rays(factor)
        got = fog_scene(placed_fog_).path_step(o, d, rng_state=states, want=want)
        ref = fog_scene(plain_fog).path_step(o, d, rng_state=states, want=want)
        inside = np.isfinite(ref["t"])
        print(f"{name}: {inside.mean():.3f} of the rays scatter in the fog")
        assert 0.2 < inside.mean() < 0.9, name
        for key in want:
            assert np.array_equal(bits(got[key]), bits(ref[key])), (name, key)
    # the two rules differ where the scale is not uniform: measured in object space, the first fog would answer otherwise
    o, d = rays(scale)
    local = fog_scene(lambda s, m: s.ConstantMedium(s.MakeBox(BOX_LO, BOX_HI, m), density, (0.8, 0.8, 0.8))).path_step(
        np.ascontiguousarray(o / scale), np.ascontiguousarray(d / scale), rng_state=states, want=want)
    world = fog_scene(cases[0][2]).path_step(o, d, rng_state=states, want=want)
    assert np.mean(local["status"] != world["status"]) > 0.02, "these rays tell the two rules apart"


# ---- 3. every route ----
def room(s, extra, world):
    """A small lit room around the placed children of section 1 (and `extra`), as a list or a BvhNode."""
    white, light = s.Lambertian((0.73, 0.73, 0.73)), s.DiffuseLight((7.0, 7.0, 7.0))
    items = [s.Quad((-6, -4, -6), (12, 0, 0), (0, 0, 12), white), s.Quad((-6, 6, -6), (12, 0, 0), (0, 0, 12), white),
             s.Quad((-6, -4, -6), (12, 0, 0), (0, 10, 0), s.Lambertian((0.12, 0.45, 0.15))),
             s.Quad((-2, 5.9, -2), (4, 0, 0), (0, 0, 4), light)]
    for k, (name, chain_name) in enumerate((("box", "shear scale rotation"), ("sphere", "mirror"), ("icosahedron", "translate transform rotate_y transform"))):
        handle, _ = tr.build_chain(s, child_of(s, name), [("translate", (-3.5 + 1.5 * k, -1.0, -2.0 + 0.5 * k))] + CHAINS[chain_name])
        items.append(handle)
    items += extra(s)
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0.0, 1.0, 14.0), (0.0, 0.5, 0.0), (0, 1, 0), 45.0, W / H, 0.0, 1.0, 0.0, 1.0, (0.1, 0.1, 0.15))
    s.Commit()
    return s


def fog_on_a_placed_box(s):   # ConstantMedium whose boundary is a Transform: an ObjectRec with a medium
    box = s.Transform(s.MakeBox(BOX_LO, BOX_HI, s.Lambertian((1, 1, 1))), affine(rotation((0, 0, 1), 20.0) @ np.diag((2.0, 3.0, 2.0)), (3.0, 0.0, 1.0)))
    return [s.ConstantMedium(box, 0.6, (0.9, 0.9, 0.9))]


def many_boxes_and_fog(s, marble=False):   # enough composite leaves for a tree of the library's own, and a medium among them
    grey = s.Lambertian(s.NoiseTexture(4.0, rt.Rng(SEED, 0))) if marble else s.Lambertian((0.4, 0.4, 0.6))
    boxes = [s.MakeBox((-5.5 + 0.9 * (k % 12), -4.0, 2.0 + 0.9 * (k // 12)), (-4.8 + 0.9 * (k % 12), -3.6 + 0.05 * (k % 5), 2.7 + 0.9 * (k // 12)), grey)
             for k in range(36)]
    return boxes + fog_on_a_placed_box(s)


def placed_fog(s):   # a ConstantMedium UNDER a Transform: the general object tree
    fog = s.ConstantMedium(s.MakeBox(BOX_LO, BOX_HI, s.Lambertian((1, 1, 1))), 1.5, (0.9, 0.9, 0.9))
    return [s.Transform(fog, affine(rotation((1, 0, 0), -25.0) @ np.diag((2.5, 2.0, 2.0)), (3.0, 0.5, 1.0)))]


ROUTES = {   # name: (extra leaves, world, render flags)
    "list world": (lambda s: [], "list", 0),
    "bvh world": (lambda s: [], "bvh", 0),
    "bvh world with a fog": (many_boxes_and_fog, "bvh", 0),
    "general kernel with a fog": (lambda s: many_boxes_and_fog(s, True), "bvh", 0),
    "object tree": (placed_fog, "bvh", 0),
    "object tree, list world": (placed_fog, "list", 0),
}


@functools.lru_cache(maxsize=None)
def route_scene(name):
    extra, world, _ = ROUTES[name]
    return room(rt.Scene(), extra, world)


@functools.lru_cache(maxsize=None)
def route_rays(name):
    arrays = camera_rays(route_scene(name))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_every_route_renders_the_one_hit_record(name):
    scene, flags = route_scene(name), ROUTES[name][2]
    o, d, tm, states = route_rays(name)
    # the specialised frame is the general one
    frame, st = scene.render(W, H, 4, seed=SEED, variant=0, flags=flags)
    general, gst = scene.render(W, H, 4, seed=SEED, variant=0, flags=flags | rt.FLAG_FORCE_GENERAL)
    print(f"{name}: kernel kind {st.kernel_kind} ({st.kernel_vgprs} VGPRs), forced general {gst.kernel_kind}; flags {scene.info()}")
    assert np.array_equal(bits(frame), bits(general))
    # a pixel of the 1-spp frame is the square root of the radiance along its camera ray from its stream
    one, _ = scene.render(W, H, 1, seed=SEED, variant=0, flags=flags)
    want = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=0, want=("radiance", "path_rays", "rng_state"))
    assert np.array_equal(bits(np.sqrt(want["radiance"])), bits(one.reshape(N, 3)))
    assert want["path_rays"].max() > 2
    # the host's fold of path steps, and the device's fold of advances
    acc, steps, final = fold(scene, o, d, tm, states, 50, {"status": set(), "material": set()})
    assert np.array_equal(bits(acc), bits(want["radiance"])) and np.array_equal(steps, want["path_rays"]) and np.array_equal(final, want["rng_state"])
    to_device = lambda a: torch.from_numpy(np.array(a)).cuda()
    batch = rt.PathBatch(scene, to_device(o), to_device(d), times=to_device(tm), rng_state=to_device(states))
    got = batch.run(50)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want["radiance"]))
    # the feature pass at the centre rays is the ray query
    co, cd, _, _ = centre_rays(scene, W, H)
    query = scene.intersect(co, cd, want=("t", "normal", "albedo", "material"), seed=SEED)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=SEED, variant=0)
    albedo, normal, depth = (p.reshape(N, -1) for p in film.features())
    assert np.array_equal(np.isfinite(query["t"]), depth[:, 0] > 0)
    assert np.array_equal(bits(query["normal"]), bits(normal)) and np.array_equal(bits(query["albedo"]), bits(albedo))
    # an adaptive film's pixel that stopped at n is the n-sample render's
    film = rt.Film(W, H)
    film.set_adaptive(4, 2, 0.35)
    ast = film.render(scene, 8, seed=SEED, variant=0, flags=flags)
    counts, pixels = film.sample_counts(), film.download()
    assert ast.kernel_kind & ADAPTIVE
    for c in np.unique(counts).tolist():
        plain, _ = scene.render(W, H, c, seed=SEED, variant=0, flags=flags)
        assert np.array_equal(bits(pixels)[counts == c], bits(plain)[counts == c]), c


def test_the_routes_are_the_kernels_they_are_named_for():
    """rt_render_stats.kernel_kind: 10 the instanced list scan, 2 the BVH walk over instances, 6 the same with media, 7 / 7 + 256 the
    general kernel, deep or segmented, 7 + 32 and 15 + 32 the general object tree under a BvhNode and a list world."""
    kinds = {name: route_scene(name).render(W, H, 1, variant=0, flags=ROUTES[name][2])[1].kernel_kind for name in sorted(ROUTES)}
    print(kinds)
    assert kinds["list world"] == 10 and kinds["bvh world"] == 2 and kinds["bvh world with a fog"] == 6
    assert kinds["general kernel with a fog"] in (7, 7 + 256)
    assert kinds["object tree"] == 7 + 32 and kinds["object tree, list world"] == 15 + 32


# ---- 4. lights ----
def lamp_room(kind):
    """A white floor under a lamp that is a quad or a triangle under a scale + a rotation (+ a translation in the same matrix)."""
    s = rt.Scene()
    light = s.DiffuseLight((9.0, 8.0, 7.0))
    lamp = s.Quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), light) if kind == "quad" else s.Triangle((-1, 0, -1), (2.5, 0, 0.2), (0.3, 0, 2.5), light)
    placed_lamp = s.Transform(s.Scale(lamp, (1.5, 1.0, 0.6)), affine(rotation((1, 0, 0.3), 160.0), (0.5, 4.0, -0.5)))
    items = [s.Quad((-8, -1, -8), (16, 0, 0), (0, 0, 16), s.Lambertian((0.7, 0.7, 0.7))), placed_lamp,
             s.Sphere((1.5, 0.0, 1.0), 1.0, s.Lambertian((0.3, 0.5, 0.8)))]
    s.SetWorld(s.HittableList(items))
    s.Camera((0.0, 3.0, 12.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0))
    s.Commit()
    return s


@pytest.mark.parametrize("kind", ["quad", "triangle"])
def test_a_lamp_under_a_transform_is_sampled_as_the_restatement_samples_its_row(kind):
    s = lamp_room(kind)
    L = s.lights()
    assert s.info()["n_lights"] == 1
    rng = np.random.default_rng(30)
    P = np.ascontiguousarray(np.stack([rng.uniform(-6, 6, 2000), np.full(2000, -1.0), rng.uniform(-6, 6, 2000)], axis=-1))
    nrm = np.ascontiguousarray(np.broadcast_to((0.0, 1.0, 0.0), P.shape))
    mat = np.zeros(len(P), dtype=np.uint8)
    states = lr.seeded_states(len(P), SEED)
    outputs = ("direction", "distance", "pdf", "light", "rng_state")
    for strategy in (0, 1):
        want = lr.sample_lights(L, P, states, strategy=strategy, normals=nrm, materials=mat)
        got = s.sample_lights(P, nrm, mat, None, states, strategy=strategy, variant=0, want=outputs)
        assert want["valid"].mean() > 0.9
        for key in outputs:
            assert np.array_equal(bits(got[key]), bits(want[key])), (strategy, key)
        d = np.ascontiguousarray(np.where(want["valid"][:, None], want["direction"], nrm))
        d[::3] = nrm[::3] + 0.2 * rng.normal(size=nrm[::3].shape)   # directions of their own as well: many miss the lamp
        pdf, light = lr.light_pdf(L, P, d, strategy=strategy)
        out = s.light_pdf(P, d, None, strategy=strategy, variant=0, want=("pdf", "light"))
        assert (light >= 0).mean() > 0.5 and (light < 0).any()
        assert np.array_equal(bits(out["pdf"]), bits(pdf)) and np.array_equal(out["light"], light)


@pytest.mark.parametrize("kind", ["quad", "triangle"])
def test_mis_and_plain_radiance_agree_under_a_placed_lamp(kind):
    """The project's criterion (tests/test_radiance_direct_gpu.py): the two estimators' means over the frame's rays within 5
    standard errors of their difference."""
    s = lamp_room(kind)
    o, d, _, _ = centre_rays(s, W, H)
    plain = s.radiance(o, d, samples=32, max_depth=8, seed=SEED, variant=0)["radiance"]
    mis = s.radiance(o, d, samples=32, max_depth=8, seed=SEED + 1, variant=0, direct="mis")["radiance"]
    diff = (mis - plain).mean(axis=-1)
    mean, se = diff.mean(), diff.std(ddof=1) / np.sqrt(len(diff))
    print(f"{kind}: plain {plain.mean():.5f}, mis {mis.mean():.5f}, difference {mean:.5f} +- {se:.5f}")
    assert plain.mean() > 0.05 and abs(mean) <= 5.0 * se


# ---- 5. scene 14 ----
def test_scene_14_renders_and_its_ellipsoid_is_glass():
    for world_kind in (0, 1):
        scene = rt.builtin_scene(14, world_kind, W, H)
        frame, st = scene.render(W, H, 8, seed=SEED, variant=0)
        general, _ = scene.render(W, H, 8, seed=SEED, variant=0, flags=rt.FLAG_FORCE_GENERAL)
        print(f"scene 14 world {world_kind}: kernel kind {st.kernel_kind}, {st.rays} rays, mean {frame.mean():.4f}")
        assert np.isfinite(frame).all() and frame.mean() > 0.02 and np.array_equal(bits(frame), bits(general))
    # the ellipsoid's centre (170, 200, 120) on the film: the pixel whose centre ray passes nearest to it
    scene = rt.builtin_scene(14, 0, W, H)
    o, d, _, _ = centre_rays(scene, W, H)
    to = np.array((170.0, 200.0, 120.0)) - o
    off = np.linalg.norm(np.cross(to, d), axis=1) / np.linalg.norm(d, axis=1)
    k = int(np.argmin(off))
    assert scene.intersect(o[k:k + 1], d[k:k + 1], want=("material",))["material"][0] == 2
    exe = os.path.join(os.path.dirname(rt.__file__), "rtow")
    out = subprocess.run([exe, "--scene", "14", "--width", str(W), "--height", str(H), "--pick", f"{k % W},{k // W}"],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout.strip())
    assert out.returncode == 0 and "dielectric" in out.stdout.lower(), out.stdout + out.stderr
