"""Triangles and triangle meshes on the GPU.  The interior rule is pinned through the quad path, which the CPU oracle pins: a
triangle (Q, u, v) and the quad (Q, u, v) share plane, t, alpha and beta bit for bit, so a triangle is hit exactly where the quad is
hit with 0 <= U, 0 <= V, fl(U + V) <= 1.  Then: every search order gives the same frame, ties between coplanar triangles keep the
reference's order, features / queries / radiance agree with each other, an icosphere lies between its inscribed and its
circumscribed sphere, and the executable renders scene 12.  Frames are at most 32 x 24 at <= 8 spp, ray sets at most about 2000."""
import functools
import os
import subprocess

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from query_helpers import bits, centre_rays, dot3, sphere_roots
from triangle_meshes import icosphere

pytestmark = pytest.mark.gpu

W, H = 32, 24
INF = float("inf")
REFERENCE = rt.FLAG_REFERENCE_TREE | rt.FLAG_FORCE_GENERAL
EDGE_BAND = 1e-9


# ---- rays ----
def pinhole_rays(origin, target, width=W, height=H, vfov=38.0, roll=0.0123):
    """Centre rays of a pinhole camera that is rolled a little about its axis, so that no row or column of them is aligned with
    anything in the scenes: (origins (N, 3), directions (N, 3)), ray k = j * width + i."""
    origin, target = np.asarray(origin, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w = (origin - target) / np.linalg.norm(origin - target)
    u = np.cross((np.sin(roll), np.cos(roll), 0.0), w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    half_h = np.tan(np.radians(vfov) / 2.0)
    half_w = half_h * width / height
    x = ((np.arange(width) + 0.5) / width * 2.0 - 1.0)[None, :, None] * half_w
    y = ((np.arange(height) + 0.5) / height * 2.0 - 1.0)[:, None, None] * half_h
    d = (x * u + y * v - w).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d)


def assert_no_centre_ray_on_an_edge(scene, width=W, height=H, what=""):
    """The reference side of a comparison of two search orders: no centre ray that hits a triangle has U, V or 1 - fl(U + V) within
    1e-9 of 0.  A triangle is a kind-4 world leaf, or lies inside a composite leaf (kind 3) and is not a medium's isotropic hit."""
    o, d, time0, _ = centre_rays(scene, width, height)
    out = scene.intersect(o, d, time=time0, want=("t", "uv", "leaf", "material"))
    kinds = scene.dump_leaves()[0]
    hit = np.isfinite(out["t"])
    tri = hit & np.isin(kinds[np.maximum(out["leaf"], 0)], (3, 4)) & (out["material"] != 4)
    assert tri.sum() > 0, f"{what}: some centre ray hits a triangle"
    uv = out["uv"][tri]
    margin = np.minimum(np.minimum(np.abs(uv[:, 0]), np.abs(uv[:, 1])), np.abs(1.0 - (uv[:, 0] + uv[:, 1])))
    print(f"{what}: {tri.sum()} of {hit.size} centre rays hit a triangle, smallest edge margin {margin.min():.3g}")
    assert margin.min() > EDGE_BAND, f"{what}: a centre ray lies on an edge"


# ---- 1, 2. the rule, pinned through the quad path ----
TRIANGLES = [   # (Q, u, v): general ones, two axis-aligned, a sliver, a degenerate one
    ((-1.913, -0.377, -3.113), (1.271, 0.219, -0.313), (0.173, 1.437, 0.291)),
    ((0.137, -0.931, -3.771), (1.613, 0.377, 0.413), (-0.291, 1.617, -0.259)),
    ((-0.713, 0.271, -2.659), (1.117, -0.433, 0.171), (0.531, 0.877, -0.613)),
    ((0.619, 0.113, -4.371), (0.871, 0.659, 0.233), (-0.977, 0.431, 0.119)),
    ((-2.231, 0.713, -4.117), (1.313, 0.117, 0.719), (0.219, -1.171, 0.331)),
    ((1.171, -1.213, -2.913), (0.733, 0.291, -0.617), (-0.413, 0.959, -0.177)),
    ((-0.331, -1.419, -2.371), (0.913, 0.071, 0.277), (0.117, 0.813, -0.391)),
    ((-1.517, -1.331, -4.713), (2.117, 0.313, 0.171), (0.419, 2.213, -0.233)),
    ((-1.373, 1.171, -3.313), (0.0, 0.0, 1.319), (1.477, 0.0, 0.0)),          # axis-aligned, in y = 1.171
    ((1.731, -0.613, -3.919), (0.0, 1.213, 0.0), (0.0, 0.0, 1.117)),          # axis-aligned, in x = 1.731
    ((-0.871, -0.171, -2.113), (1.713, 0.319, 0.233), (1.697, 0.331, 0.229)),  # a sliver
    ((0.213, 0.517, -2.517), (0.619, 0.213, -0.117), (1.238, 0.426, -0.234)),  # degenerate: v = 2 u
]
CAMERAS = [((0.0213, 0.0371, 1.0117), (0.0, 0.0, -3.2)), ((2.913, 1.371, 0.517), (-0.2, 0.1, -3.4))]
TURN, SHIFT = 23.7, (0.319, -0.213, 0.171)   # the instance of the third world: RotateY then Translate


def instance_points(p):
    """Points of the instanced list in world space (Translate(RotateY(.))): only used to aim rays."""
    a = np.radians(TURN)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([np.cos(a) * x + np.sin(a) * z, y, -np.sin(a) * x + np.cos(a) * z], axis=-1) + SHIFT


def pinned_rays(instanced, edges=True, inside_boxes=False):
    """The 32 x 24 centre rays of two cameras, and from each camera a ray at every corner, edge midpoint and edge quarter point of
    every triangle as computed: there the rule is decided by rounding.  ``inside_boxes`` (the BVH world) leaves out the points
    that lie ON a face of their triangle's bounding box -- every corner that is an extreme of the three, every point of an edge
    along an axis: whether a tree's slab test (R/AABB.h) passes a ray through such a point is decided by the rounding of the BOX
    test, which a list does not make; the rule under test is decided behind it.  The BVH world aims at a third point of every
    edge instead (3/8 along it), so that it too has about 200 rays where rounding decides: AIMED has the counts."""
    o, d = zip(*(pinhole_rays(*cam) for cam in CAMERAS))
    o, d = list(o), list(d)
    if edges:
        pts = []
        for q, u, v in TRIANGLES:
            a, b, c = np.array(q), np.array(q) + u, np.array(q) + v
            lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
            for p0, p1 in ((a, b), (b, c), (c, a)):
                for p in (p0, 0.5 * (p0 + p1), 0.25 * p0 + 0.75 * p1) + ((0.625 * p0 + 0.375 * p1,) if inside_boxes else ()):
                    thin = hi - lo < 1e-4   # (a thin axis is padded by the box: the point lies inside there)
                    if not inside_boxes or not np.any(((p <= lo) | (p >= hi)) & ~thin):
                        pts.append(p)
        pts = np.array(pts)
        if instanced:
            pts = instance_points(pts)
        for origin, _ in CAMERAS:
            o.append(np.broadcast_to(np.asarray(origin), pts.shape))
            d.append(pts - origin)
    return np.ascontiguousarray(np.concatenate(o)), np.ascontiguousarray(np.concatenate(d))


AIMED = {"list": 216, "instanced list": 216, "bvh": 196}   # rays aimed at edges and corners (bvh: see pinned_rays)


def pinned_world(kind):
    """(scene, position in the triangle list of every world leaf's triangle or None)."""
    s = rt.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    tris = [s.Triangle(q, u, v, m) for q, u, v in TRIANGLES]
    if kind == "list":
        s.SetWorld(s.HittableList(tris))
        order = list(range(len(tris)))
    elif kind == "bvh":
        sorted_tris = list(tris)
        s.SetWorld(s.BvhNode(sorted_tris))
        order = [tris.index(h) for h in sorted_tris]
    else:
        s.SetWorld(s.HittableList([s.Translate(s.RotateY(s.HittableList(tris), TURN), SHIFT)]))
        order = None
    s.Camera(CAMERAS[0][0], CAMERAS[0][1], (0, 1, 0), 38.0, W / H, 0.0, 1.0)
    s.Commit()
    return s, order


@functools.lru_cache(maxsize=None)
def quad_answers(instanced, variant, edges, inside_boxes=False):
    """For every triangle i the one-leaf scene of the quad (Q_i, u_i, v_i) under the same transform, every quad on the general
    test (RT_SCENE_PLAIN_QUADS), asked for t, uv, normal and front_face along the pinned rays.  Computed once, never written to."""
    o, d = pinned_rays(instanced, edges, inside_boxes)
    answers = []
    for q, u, v in TRIANGLES:
        s = rt.Scene()
        s.set_options(rt.SCENE_PLAIN_QUADS)
        quad = s.Quad(q, u, v, s.Lambertian((0.5, 0.5, 0.5)))
        s.SetWorld(s.HittableList([s.Translate(s.RotateY(s.HittableList([quad]), TURN), SHIFT) if instanced else quad]))
        s.Camera(CAMERAS[0][0], CAMERAS[0][1], (0, 1, 0), 38.0, W / H, 0.0, 1.0)
        s.Commit()
        out = s.intersect(o, d, variant=variant, want=("t", "uv", "normal", "front_face"))
        for a in out.values():
            a.setflags(write=False)
        answers.append(out)
    return answers


def list_rule(answers):
    """R/HittableList.h:39-57 over the triangles in list order: triangle i is hit where its quad is hit with 0 <= U, 0 <= V and
    fl(U + V) <= 1; a later hit with t <= the closest so far replaces it (R/Quad.h:59 is inclusive).  Returns (winner per ray or -1,
    t, uv, normal, front_face, the number of triangles hit per ray at the winning t)."""
    n = answers[0]["t"].shape[0]
    winner, t = np.full(n, -1), np.full(n, INF)
    uv, normal, front = np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    hits = []
    for i, a in enumerate(answers):
        U, V = a["uv"][:, 0], a["uv"][:, 1]
        hit = np.isfinite(a["t"]) & (U >= 0) & (V >= 0) & (np.float64(U) + np.float64(V) <= 1)
        hits.append(np.where(hit, a["t"], np.nan))
        take = hit & (a["t"] <= t)
        winner[take], t[take] = i, a["t"][take]
        uv[take], normal[take], front[take] = a["uv"][take], a["normal"][take], a["front_face"][take]
    with np.errstate(invalid="ignore"):
        at_best = np.sum(np.array(hits) == t[None, :], axis=0)
    return winner, t, uv, normal, front, at_best


@pytest.mark.parametrize("kind", ["list", "bvh", "instanced list"])
def test_strict_triangles_are_the_quads_with_the_triangle_rule_bit_for_bit(kind):
    instanced = kind == "instanced list"
    scene, order = pinned_world(kind)
    o, d = pinned_rays(instanced, inside_boxes=kind == "bvh")
    answers = quad_answers(instanced, 0, True, kind == "bvh")
    winner, t, uv, normal, front, at_best = list_rule(answers)
    hit = winner >= 0
    quad_only = sum(int(np.sum(np.isfinite(a["t"]))) for a in answers) - int(np.sum(at_best))
    print(f"{kind}: {o.shape[0]} rays ({o.shape[0] - 2 * W * H} aimed at edges and corners), {hit.sum()} hit a triangle; "
          f"{quad_only} quad hits fall outside their triangle; degenerate quad hit by {np.isfinite(answers[11]['t']).sum()}")
    assert o.shape[0] - 2 * W * H == AIMED[kind] and o.shape[0] <= 2000 and hit.sum() > 300 and quad_only > 100
    assert not np.isfinite(answers[11]["t"]).any(), "the degenerate quad is never hit"
    assert len(set(winner[hit])) == 11, "every triangle but the degenerate one wins some ray"
    if kind == "bvh":
        assert at_best.max() == 1, "no ray meets two triangles at one t: the order of a tree's tests then decides nothing"
    got = scene.intersect(o, d, variant=0, want=("t", "uv", "normal", "front_face", "leaf", "occluded"))
    wrong = np.flatnonzero(bits(got["t"]) != bits(t))
    print(f"    t differs for {wrong.size} rays: {[(int(k), float(got['t'][k]), float(t[k]), int(winner[k])) for k in wrong[:12]]}")
    assert np.array_equal(np.isfinite(got["t"]), hit)
    assert np.array_equal(bits(got["t"]), bits(t))
    assert np.array_equal(bits(got["uv"]), bits(uv))
    assert np.array_equal(bits(got["normal"]), bits(normal))
    assert np.array_equal(got["front_face"], front)
    if order is None:
        want_leaf = np.where(hit, 0, -1)
    else:
        position = np.array([order.index(i) for i in range(len(TRIANGLES))])
        want_leaf = np.where(hit, position[np.maximum(winner, 0)], -1)
    assert np.array_equal(got["leaf"], want_leaf)
    assert np.array_equal(got["occluded"] != 0, hit)
    assert np.array_equal(scene.occluded(o, d, variant=0), hit)


@pytest.mark.parametrize("kind", ["list", "bvh", "instanced list"])
def test_fast_triangles_are_the_fast_quads_with_the_triangle_rule(kind):
    instanced = kind == "instanced list"
    scene, order = pinned_world(kind)
    o, d = pinned_rays(instanced, edges=False)
    answers = quad_answers(instanced, 1, False)
    winner, t, uv, normal, front, at_best = list_rule(answers)
    # the band: rays of which some quad's U, V or fl(U + V) - 1 lies within 1e-9 of the rule's bounds
    near = np.zeros(o.shape[0], dtype=bool)
    for a in answers:
        U, V = a["uv"][:, 0], a["uv"][:, 1]
        near |= np.isfinite(a["t"]) & ((np.abs(U) <= EDGE_BAND) | (np.abs(V) <= EDGE_BAND) | (np.abs((U + V) - 1.0) <= EDGE_BAND))
    print(f"{kind}: {near.sum()} of {near.size} rays inside the band")
    assert near.mean() <= 0.01 and near.sum() == 0, "the centre rays of the two cameras keep away from every edge"
    got = scene.intersect(o, d, variant=1, want=("t", "uv", "leaf"))
    hit = winner >= 0
    assert np.array_equal(np.isfinite(got["t"]), hit)
    rel_t = np.abs(got["t"][hit] - t[hit]) / np.abs(t[hit])
    rel_uv = np.abs(got["uv"][hit] - uv[hit]) / np.abs(uv[hit])
    print(f"    t: worst relative difference {rel_t.max():.3g}; uv: {rel_uv.max():.3g}")
    assert rel_t.max() <= 1e-12 and rel_uv.max() <= 1e-12
    if order is not None:
        position = np.array([order.index(i) for i in range(len(TRIANGLES))])
        assert np.array_equal(got["leaf"], np.where(hit, position[np.maximum(winner, 0)], -1))


# ---- 3. every search agrees ----
def two_icosahedra(s, world, with_spheres=True):
    """40 triangles as world leaves of their own (two icosahedra side by side, nothing coplanar between them), among five spheres."""
    items = []
    for centre, radius, colour in (((-0.613, 0.071, -0.117), 0.571, (0.8, 0.3, 0.2)), ((0.719, -0.113, 0.233), 0.619, (0.2, 0.4, 0.8))):
        verts, faces = icosphere(0, radius)
        items += s.TriangleMesh(verts + centre, faces, s.Lambertian(colour), return_triangles=True)[1]
    if with_spheres:
        items += [s.Sphere((0.0, -100.7, 0.0), 100.0, s.Lambertian((0.5, 0.6, 0.4))), s.Sphere((0.05, 0.9, -0.3), 0.25, s.Metal((0.8, 0.8, 0.8), 0.1)),
                  s.Sphere((-1.5, 0.3, 0.4), 0.3, s.Dielectric(1.5)), s.Sphere((1.7, 0.2, -0.5), 0.3, s.Lambertian((0.7, 0.7, 0.2))),
                  s.Sphere((0.1, 0.0, 1.1), 0.2, s.DiffuseLight((4.0, 4.0, 4.0)))]
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0.313, 1.171, 3.719), (0.0, 0.0, 0.0), (0.0123, 1.0, 0.0), 36.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


def few_leaves(s):
    """A BVH world of 14 leaves: few enough for the launcher to scan them instead of walking."""
    verts, faces = icosphere(0, 0.613)
    items = s.TriangleMesh(verts + (0.113, 0.071, -0.031), faces[:10], s.Lambertian((0.8, 0.3, 0.2)), return_triangles=True)[1]
    items += [s.Sphere((0.0, -100.7, 0.0), 100.0, s.Lambertian((0.5, 0.6, 0.4))), s.Sphere((0.05, 0.9, -0.3), 0.25, s.Metal((0.8, 0.8, 0.8), 0.1)),
              s.Sphere((-1.1, 0.3, 0.4), 0.3, s.Dielectric(1.5)), s.Sphere((1.2, 0.2, -0.5), 0.3, s.Lambertian((0.7, 0.7, 0.2)))]
    s.SetWorld(s.BvhNode(items))
    s.Camera((0.313, 1.171, 3.719), (0.0, 0.0, 0.0), (0.0123, 1.0, 0.0), 36.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


def cornell_meshes(s, extra):
    """Scene 12's walls, light, camera and meshes, built through the Python API, plus what ``extra(s, white)`` returns."""
    red, white, green = s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.12, 0.45, 0.15))
    light = s.DiffuseLight((15.0, 15.0, 15.0))
    items = [s.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green), s.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),
             s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), light), s.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),
             s.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white), s.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)]
    ball = s.TriangleMesh(*icosphere(2, 100.0), white)
    solid = s.TriangleMesh(*icosphere(0, 90.0), s.Metal((0.8, 0.85, 0.88), 0.0))
    items += [s.Translate(ball, (347.5, 100.0, 377.5)), s.Translate(s.RotateY(solid, -18.0), (212.5, 90.0, 147.5))]
    items += extra(s, white)
    s.SetWorld(s.BvhNode(items))
    s.Camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 0.0, (0, 0, 0))
    s.Commit()
    return s


def with_medium_sphere():
    return cornell_meshes(rt.Scene(), lambda s, white: [s.ConstantMedium(s.Sphere((130.0, 330.0, 250.0), 90.0, white), 0.01, (0.9, 0.9, 0.9))])


def deep_rich_world():
    """The meshes and the medium sphere in a world the launcher calls deep and rich: 80 more leaves (more than 64 world nodes),
    half of them of a NoiseTexture.  Such a world takes the segmented walk over the library's tree of the surface leaves (C5's
    kernel), the instanced meshes among them; with RT_FLAG_REFERENCE_TREE the deep general kernel over the reference's tree."""
    def extra(s, white):
        marble = s.Lambertian(s.NoiseTexture(0.05, rt.Rng(1984, 0)))
        rng = np.random.default_rng(12)
        items = [s.ConstantMedium(s.Sphere((130.0, 330.0, 250.0), 90.0, white), 0.01, (0.9, 0.9, 0.9))]
        for k in range(80):
            x, z = 30.0 + 55.0 * (k % 10) + rng.uniform(0, 9), 30.0 + 60.0 * (k // 10) + rng.uniform(0, 9)
            items.append(s.Sphere((x, 12.0 + rng.uniform(0, 3), z), 12.0, marble if k % 2 else white))
        return items
    return cornell_meshes(rt.Scene(), extra)


def icosahedron_of_smoke(medium=True):
    def extra(s, white):
        shell = s.TriangleMesh(*icosphere(0, 95.0), white)
        return [s.Translate(s.ConstantMedium(shell, 0.02, (0.9, 0.9, 0.9)) if medium else shell, (130.0, 400.0, 250.0))]
    return cornell_meshes(rt.Scene(), extra)


def nested_list(tree=True):
    """A rotated icosahedron mesh and a sphere in one list under a Translate.  A list of composites inside an instance is more than
    an object record holds: the world keeps it as an object tree for the interpreter (tree_hit).  Its flat twin gives each of the
    two its own chain of the same transforms -- the same local rays, the same tests -- and is searched by the instance kernels."""
    def extra(s, white):
        shell, ball = s.TriangleMesh(*icosphere(0, 95.0), white), s.Sphere((40.0, 120.0, -30.0), 35.0, s.Metal((0.8, 0.8, 0.8), 0.0))
        offset = (130.0, 400.0, 250.0)
        if tree:
            return [s.Translate(s.HittableList([s.RotateY(shell, 21.0), ball]), offset)]
        return [s.Translate(s.RotateY(shell, 21.0), offset), s.Translate(ball, offset)]
    return cornell_meshes(rt.Scene(), extra)


# kernel kinds (rt_render_stats.kernel_kind; tests/test_launch_plan.py pins the planner's own table)
GENERAL_BVH, GENERAL_LIST, NESTED_BVH, SEGMENTED, ADAPTIVE = 7, 15, 39, 263, 512
SEARCHES = {
    # name: (scene, the scene whose centre rays are checked or None for the scene itself, the scene of the reference frame or None,
    #        spp, kind of the reference frame, [(render keywords, kind) of the frames that must equal the reference's])
    "40 triangles and spheres, bvh": (lambda: two_icosahedra(rt.Scene(), "bvh"), None, None, 4, GENERAL_BVH, [({}, 64)]),   # library tree
    "40 triangles and spheres, list": (lambda: two_icosahedra(rt.Scene(), "list"), None, None, 4, GENERAL_LIST,
                                       [({}, 8), ({"flags": rt.FLAG_ACCELERATE_LISTS}, 64), ({"pixels_per_wave": 8}, 136)]),
    "14 leaves": (lambda: few_leaves(rt.Scene()), None, None, 4, GENERAL_BVH,
                  [({}, 8), ({"flags": rt.FLAG_ALWAYS_WALK}, 64), ({"pixels_per_wave": 8}, 136)]),   # scan, walk, grouped scan
    "scene 12 bvh": (lambda: rt.builtin_scene(12, 0, W, H), None, None, 4, GENERAL_BVH, [({}, 2)]),
    "scene 12 list": (lambda: rt.builtin_scene(12, 1, W, H), None, None, 4, GENERAL_LIST, [({}, 10), ({"pixels_per_wave": 8}, 138)]),
    "meshes and a medium sphere": (with_medium_sphere, None, None, 4, GENERAL_BVH, [({}, 6)]),
    "meshes, a medium sphere and marble: deep": (deep_rich_world, None, None, 4, GENERAL_BVH, [({}, SEGMENTED)]),
    # every launch of a world with an object tree runs the interpreter's kernel, the reference's flags included: the frames of this
    # case are one kernel's twice (that it runs the rule at all, and reproducibly); "a nested list" below has a partner
    "a medium inside an icosahedron": (icosahedron_of_smoke, lambda: icosahedron_of_smoke(medium=False), None, 4, NESTED_BVH, [({}, NESTED_BVH)]),
    "a nested list": (nested_list, lambda: nested_list(tree=False), lambda: nested_list(tree=False), 4, GENERAL_BVH, [({}, NESTED_BVH)]),
    "scene 12 bvh, adaptive": (lambda: rt.builtin_scene(12, 0, W, H), None, None, 8, GENERAL_BVH + ADAPTIVE,
                               [({"adaptive": (4, 2, 0.05)}, 2 + ADAPTIVE)]),
}


@pytest.mark.parametrize("name", sorted(SEARCHES))
def test_every_search_gives_the_reference_trees_frame_bit_for_bit(name):
    make, make_twin, make_reference, spp, reference_kind, variations = SEARCHES[name]
    scene = make()
    reference = scene if make_reference is None else make_reference()
    assert_no_centre_ray_on_an_edge(scene if make_twin is None else make_twin(), what=name)
    info = scene.info()
    print(f"{name}: {info['n_triangles']} triangles, {info['n_leaves']} leaves, {info['n_objects']} objects, {info['n_nodes']} threaded nodes, "
          f"{scene.dump_fast_nodes()[0].shape[0]} nodes in the library's tree")
    if name == "40 triangles and spheres, bvh":
        assert scene.dump_fast_nodes()[0].shape[0] > 0 and info["n_triangles"] == 40
    for kw, kind in variations:
        base = {k: v for k, v in kw.items() if k == "adaptive"}
        want, want_st = reference.render(W, H, spp, variant=0, flags=REFERENCE, **base)
        got, st = scene.render(W, H, spp, variant=0, **kw)
        differ = int(np.sum((bits(got) != bits(want)).any(axis=-1)))
        print(f"    {kw}: kernel kind {st.kernel_kind} against {want_st.kernel_kind}, {differ} of {W * H} pixels differ")
        assert (st.kernel_kind, want_st.kernel_kind) == (kind, reference_kind), "the searches this case is about"
        assert want.max() > 0 and differ == 0, (name, kw)
        if "adaptive" in kw:
            counts = st.sample_counts
            assert counts.min() < counts.max(), "some pixels stop early, some do not"


# ---- 4. ties ----
@pytest.mark.parametrize("side", ["above", "below"])
def test_coplanar_triangles_of_two_leaves_keep_the_reference_trees_order(side):
    s = rt.Scene()
    red, blue = s.Lambertian((0.9, 0.1, 0.1)), s.Lambertian((0.1, 0.1, 0.9))
    items = [s.Triangle((-1.0, 0.0, -1.0), (2.5, 0.0, 0.0), (0.0, 0.0, 2.5), red), s.Triangle((-0.5, 0.0, -0.75), (2.5, 0.0, 0.0), (0.0, 0.0, 2.5), blue)]
    items += [s.Sphere((-1.7 + 0.7 * k, 0.35 if k % 2 else -0.35, -1.3), 0.2, s.Metal((0.8, 0.8, 0.8), 0.0)) for k in range(6)]
    s.SetWorld(s.BvhNode(items))
    y = 2.913 if side == "above" else -2.913
    s.Camera((0.319, y, 3.117), (0.0, 0.0, 0.0), (0.0123, 1.0, 0.0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    assert s.dump_fast_nodes()[0].shape[0] == 0, "the guard finds the shared area"
    o, d, time0, _ = centre_rays(s, W, H)
    first = s.intersect(o, d, time=time0, want=("t", "leaf", "albedo"))
    both = int(np.sum(np.isfinite(first["t"]) & (first["albedo"][:, 1] == 0.1)))
    print(f"{side}: {both} centre rays end on one of the two triangles")
    assert both > 50
    want, _ = s.render(W, H, 4, variant=0, flags=rt.FLAG_REFERENCE_TREE)
    got, _ = s.render(W, H, 4, variant=0)
    assert np.array_equal(bits(got), bits(want))


# ---- 5. queries and features ----
@pytest.mark.parametrize("world", [0, 1], ids=["bvh", "list"])
def test_scene_12_feature_pass_equals_the_closest_hit_query(world):
    scene = rt.builtin_scene(12, world, W, H)
    o, d, time0, _ = centre_rays(scene, W, H)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=1984, variant=0)
    albedo, normal, depth = (p.reshape(W * H, -1) for p in film.features())
    got = scene.intersect(o, d, time=time0, variant=0, want=("t", "normal", "albedo", "leaf", "uv"))
    hit = np.isfinite(got["t"])
    assert 0.5 < hit.mean() < 1.0 and np.array_equal(hit, depth[:, 0] > 0), "the room is open towards the camera: the outer columns miss"
    assert np.array_equal(bits(got["normal"]), bits(normal)) and np.array_equal(bits(got["albedo"]), bits(albedo))
    rel = np.abs(got["t"][hit] * np.sqrt(dot3(d, d))[hit] - depth[hit, 0]) / depth[hit, 0]
    assert rel.max() <= 1e-15
    on_mesh = hit & (scene.dump_leaves()[0][np.maximum(got["leaf"], 0)] == 3)
    print(f"{on_mesh.sum()} centre rays end on a mesh")
    assert on_mesh.sum() > 40
    uv = got["uv"][on_mesh]
    assert (uv >= 0).all() and (uv[:, 0] + uv[:, 1] <= 1).all(), "barycentric coordinates of a triangle"


def test_triangle_normals_are_unit_and_perpendicular_to_the_edges():
    scene, _ = pinned_world("list")
    o, d = pinned_rays(False, edges=False)
    got = scene.intersect(o, d, want=("t", "normal", "leaf", "front_face"))
    hit = np.isfinite(got["t"])
    n = got["normal"][hit]
    u = np.array([TRIANGLES[i][1] for i in got["leaf"][hit]])
    v = np.array([TRIANGLES[i][2] for i in got["leaf"][hit]])
    unit = np.abs(np.sqrt(dot3(n, n)) - 1.0)
    along = np.maximum(np.abs(dot3(n, u)) / np.sqrt(dot3(u, u)), np.abs(dot3(n, v)) / np.sqrt(dot3(v, v)))
    print(f"{hit.sum()} hits: |n| - 1 at most {unit.max():.3g}, n . edge at most {along.max():.3g}")
    assert hit.sum() > 300 and unit.max() <= 1e-12 and along.max() <= 1e-12
    assert (dot3(d[hit], n) < 0).all(), "faced against the ray"
    assert np.array_equal(got["front_face"][hit] != 0, dot3(d[hit], np.cross(u, v)) < 0), "front face: the ray meets the side u x v points to"


class Stream:
    """A pixel's XORWOW stream continued from its six state words (csrc/rng.h: d, v0 .. v4)."""

    def __init__(self, words):
        self.d, self.v = int(words[0]), [int(w) for w in words[1:]]

    def uniform(self):
        v, m = self.v, 0xFFFFFFFF
        t = v[0] ^ (v[0] >> 2)
        v[:] = v[1:] + [((v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))) & m]
        self.d = (self.d + 362437) & m
        return np.float32((v[4] + self.d) & m) * np.float32(2.3283064e-10) + np.float32(2.3283064e-10) / np.float32(2.0)

    def state(self):
        return [self.d] + self.v


def next_camera_rays(scene, states, width, height):
    """The next camera ray of every pixel drawn from its stream, in camera_ray's order of draws and operations
    (tests/test_radiance_gpu.py camera_rays), and the streams after those draws."""
    cam = scene.dump_camera()
    origin, llc, hor, ver, cam_u, cam_v = (cam[3 * k:3 * k + 3] for k in (1, 2, 3, 4, 5, 6))
    lens_radius, time0, time1 = cam[24], cam[25], cam[26]
    n = width * height
    o, d, tm, out = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros((n, 6), dtype=np.uint32)
    for k in range(n):
        i, j = k % width, k // width
        rng = Stream(states[k])
        u = np.float64(np.float32(i) + rng.uniform()) / np.float64(width)
        v = np.float64(np.float32(j) + rng.uniform()) / np.float64(height)
        while True:
            a, b = np.float64(rng.uniform()), np.float64(rng.uniform())
            p = 2.0 * np.array([a, b, 0.0]) - np.array([1.0, 1.0, 0.0])
            if p[0] * p[0] + p[1] * p[1] + p[2] * p[2] < 1.0:
                break
        rd = lens_radius * p
        offset = rd[0] * cam_u + rd[1] * cam_v
        tm[k] = time0 + np.float64(rng.uniform()) * (time1 - time0)
        o[k] = origin + offset
        d[k] = (((llc + u * hor) + v * ver) - origin) - offset
        out[k] = rng.state()
    return o, d, tm, out


def test_a_film_of_scene_12_is_the_square_root_of_the_radiance_of_its_camera_rays():
    w = h = 16
    spp = 4
    scene = rt.builtin_scene(12, 0, w, h)
    film = rt.Film(w, h)
    film.render(scene, spp, max_depth=50, seed=1984, variant=0)
    pixels = film.download().reshape(w * h, 3)
    states = np.array([rt.Rng(1984, k).state() for k in range(w * h)], dtype=np.uint32)
    assert Stream(states[5]).uniform() == np.float32(rt.Rng(1984, 5).uniform()), "the host restatement of the stream"
    total = np.zeros((w * h, 3))
    for _ in range(spp):
        o, d, tm, states = next_camera_rays(scene, states, w, h)
        out = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=0, want=("radiance", "rng_state"))
        total = total + out["radiance"]
        states = np.ascontiguousarray(out["rng_state"])
    want = np.sqrt((1.0 / spp) * total)
    differ = int(np.sum((bits(want) != bits(pixels)).any(axis=-1)))
    print(f"{differ} of {w * h} pixels differ")
    assert pixels.max() > 0 and differ == 0


# ---- 6. an oracle that owes nothing to this code ----
@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_an_icosphere_lies_between_its_inscribed_and_its_circumscribed_sphere(variant):
    radius, centre = 1.0, np.array([0.0713, -0.0319, -3.0117])
    verts, faces = icosphere(3, radius)
    assert faces.shape[0] == 1280
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = np.cross(b - a, c - a)
    inner = float(np.min(np.abs(dot3(n, a)) / np.sqrt(dot3(n, n))))   # the smallest distance of a face plane from the centre
    print(f"R_in = {inner:.6f} R")
    assert 0.98 < inner < radius
    s = rt.Scene()
    s.SetWorld(s.TriangleMesh(verts + centre, faces, s.Lambertian((0.5, 0.5, 0.5))))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    o, d = pinhole_rays((0.0113, 0.0071, 0.0), (0.0, 0.0, -3.0), vfov=40.0)
    t_mesh = s.intersect(o, d, variant=variant, want=("t",))["t"]
    t_out, t_in = sphere_roots(o, d, centre, radius)[0], sphere_roots(o, d, centre, inner)[0]   # near roots, NaN for a miss
    mesh, outer, inside = np.isfinite(t_mesh), np.isfinite(t_out), np.isfinite(t_in)
    print(f"{inside.sum()} rays hit the inscribed sphere, {mesh.sum()} the mesh, {outer.sum()} the circumscribed sphere")
    assert inside.sum() > 150
    assert (mesh[inside]).all(), "a ray through the inscribed sphere cannot pass between the faces"
    assert (outer[mesh]).all(), "no face reaches outside the circumscribed sphere"
    assert (t_out[inside] <= t_mesh[inside] * (1 + 1e-12)).all() and (t_mesh[inside] <= t_in[inside] * (1 + 1e-12)).all()
    assert np.array_equal(s.occluded(o, d, variant=variant), mesh)


# ---- 7. the executable ----
def test_rtow_renders_scene_12(tmp_path):
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    out, want = tmp_path / "scene12.ppm", tmp_path / "api.ppm"
    run = subprocess.run([exe, "--scene", "12", "--width", "32", "--height", "32", "--spp", "2", "--output", str(out)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    frame, _ = rt.builtin_scene(12, 0, 32, 32).render(32, 32, 2, variant=1)
    rt.write_ppm(want, frame)
    assert out.read_bytes() == want.read_bytes()
