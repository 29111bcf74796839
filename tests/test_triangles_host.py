"""Triangles and triangle meshes on the host: construction, bounding boxes, argument checks, what commit makes of them (leaf
kinds, the launch plan, the tie guard's decision on coplanar faces) and the OBJ reader.  No GPU needed."""
import ctypes as C
import time

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib
from frame_helpers import render_params
from triangle_meshes import corners, icosphere, lattice

RT_ERR_INVALID = 1
W, H = 32, 24


def scene_with(build, world="bvh"):
    """A committed scene whose world holds the hittables ``build(s)`` returns."""
    s = rt.Scene()
    items = build(s)
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0.31, 3.7, 4.9), (0.5, 0, 0.5), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


def has_library_tree(s):
    return s.dump_fast_nodes()[0].shape[0] > 0


# ---- bounding box ----
def test_box_of_a_general_triangle_is_the_min_and_max_of_its_three_computed_corners():
    s = rt.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    for q, u, v in [((0.137, -2.31, 4.771), (1.913, 0.377, -0.613), (-0.291, 2.117, 0.859)),
                    ((1e3 + 0.1, 0.3, -7.7), (0.1, 0.2, 0.3), (-0.3, 0.1, 0.2)),
                    ((0.25, 0.5, 0.75), (0.0, 1.5, 0.25), (2.0, -0.5, 0.125))]:   # u has no x extent, the triangle has
        c = corners(q, u, v)
        box = np.array(s.BoundingBox(s.Triangle(q, u, v, m))).reshape(3, 2)
        assert np.array_equal(box[:, 0], c.min(axis=0)) and np.array_equal(box[:, 1], c.max(axis=0))


@pytest.mark.parametrize("q,u,v,thin", [((0.3, 1.25, -0.7), (2.0, 0, 0), (0, 0, 1.5), 1), ((0.3, 1.25, -0.7), (0, 0, -2.0), (0, 1.5, 0), 0),
                                        ((-4.0, 0.5, 9.0), (0, 3.0, 0), (1.0, 0, 0), 2)])
def test_an_axis_aligned_triangle_gets_the_quads_thin_axis_padding(q, u, v, thin):
    s = rt.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    tri = np.array(s.BoundingBox(s.Triangle(q, u, v, m))).reshape(3, 2)
    quad = np.array(s.BoundingBox(s.Quad(q, u, v, m))).reshape(3, 2)
    assert np.array_equal(tri[thin], quad[thin]) and tri[thin, 1] - tri[thin, 0] > 0.9e-4
    c = corners(q, u, v)
    for k in range(3):
        if k != thin:
            assert tri[k, 0] == c[:, k].min() and tri[k, 1] == c[:, k].max()


# ---- argument checks ----
def test_every_refusal_and_the_order_of_triangles_out():
    s = rt.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    L = rt.lib()
    v3 = lambda *a: (C.c_double * 3)(*a)
    assert L.rt_triangle(s._p, v3(0, 0, 0), v3(1, 0, 0), v3(0, 1, 0), 99) == 0, "invalid material"
    assert L.rt_triangle(s._p, None, v3(1, 0, 0), v3(0, 1, 0), m) == 0 and L.rt_triangle(s._p, v3(0, 0, 0), None, v3(0, 1, 0), m) == 0
    assert L.rt_triangle(s._p, v3(0, 0, 0), v3(1, 0, 0), None, m) == 0
    with pytest.raises(rt.RtowError):
        s.Triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 99)

    verts, faces = icosphere(0, 1.0)
    vp, fp = verts.ctypes.data_as(_lib.D3), faces.ctypes.data_as(C.POINTER(C.c_int32))
    mesh = lambda vptr, nv, fptr, nf, mat=m: L.rt_triangle_mesh(s._p, vptr, nv, fptr, nf, mat, None)
    assert mesh(vp, 12, fp, 0) == 0 and mesh(vp, 12, fp, -1) == 0, "n_triangles < 1"
    assert mesh(vp, 2, fp, 20) == 0, "n_vertices < 3"
    assert mesh(None, 12, fp, 20) == 0 and mesh(vp, 12, None, 20) == 0, "a NULL array"
    assert mesh(vp, 12, fp, 20, 99) == 0, "invalid material"
    assert mesh(vp, 11, fp, 20) == 0, "an index at n_vertices"
    low = faces.copy()
    low[7, 1] = -1
    assert mesh(vp, 12, low.ctypes.data_as(C.POINTER(C.c_int32)), 20) == 0, "a negative index"
    for bad in (low, np.zeros((0, 3), dtype=np.int32)):
        with pytest.raises(rt.RtowError):
            s.TriangleMesh(verts, bad, m)

    # triangles_out in input order, whatever order the BvhNode sorted its own copy into; the mesh's box is their union
    root, tris = s.TriangleMesh(verts, faces, m, return_triangles=True)
    assert len(tris) == 20
    boxes = np.array([s.BoundingBox(t) for t in tris]).reshape(20, 3, 2)
    for k, (a, b, c) in enumerate(faces):
        want = corners(verts[a], verts[b] - verts[a], verts[c] - verts[a])
        assert np.array_equal(boxes[k, :, 0], want.min(axis=0)) and np.array_equal(boxes[k, :, 1], want.max(axis=0)), k
    union = np.array(s.BoundingBox(root)).reshape(3, 2)
    assert np.array_equal(union[:, 0], boxes[:, :, 0].min(axis=0)) and np.array_equal(union[:, 1], boxes[:, :, 1].max(axis=0))


# ---- leaves and info ----
def test_a_mesh_as_the_world_reports_triangle_leaves_and_their_count():
    verts, faces = icosphere(1, 1.5)
    s = rt.Scene()
    s.SetWorld(s.TriangleMesh(verts + (0.5, 0.2, 0.5), faces, s.Lambertian((0.5, 0.5, 0.5))))
    s.Camera((0.31, 3.7, 4.9), (0.5, 0, 0.5), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    kinds, boxes = s.dump_leaves()
    info = s.info()
    assert kinds.shape == (80,) and (kinds == 4).all()
    assert info["n_triangles"] == 80 and info["n_quads"] == 80 and info["n_leaves"] == 80 and info["world_kind"] == 0
    assert C.sizeof(_lib.SceneInfo) == 18 * 4, "rt_scene_info keeps its size"
    quads = scene_with(lambda q: [q.Quad((k, 0, 0), (0.5, 0, 0), (0, 0.5, 0.1), q.Lambertian((0.5, 0.5, 0.5))) for k in range(5)])
    assert quads.info()["n_triangles"] == 0 and (quads.dump_leaves()[0] == 2).all()
    assert rt.builtin_scene(12, 0, W, H).info()["n_triangles"] == 340 and rt.builtin_scene(7, 0, W, H).info()["n_triangles"] == 0


# ---- planning ----
def _twenty_four(shape):
    def build(s):
        m = s.Lambertian((0.5, 0.5, 0.5))
        rng = np.random.default_rng(7)
        make = s.Triangle if shape == "triangle" else s.Quad
        return [make(rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), m) for _ in range(24)]
    return build


@pytest.mark.parametrize("world", ["list", "bvh"])
@pytest.mark.parametrize("flags", [0, rt.FLAG_REFERENCE_TREE, rt.FLAG_ACCELERATE_LISTS, rt.FLAG_FORCE_GENERAL])
def test_a_world_of_triangles_plans_to_the_kernel_of_the_same_world_of_quads(world, flags):
    plans = []
    for shape in ("triangle", "quad"):
        s = scene_with(_twenty_four(shape), world)
        plans.append(s.plan_launch(render_params(400, 300, 16, flags=flags), num_cus=256))
    tri, quad = plans
    for key in ("kernel_kind", "kernel", "waves_per_simd", "reference_tree"):   # (the trees differ: a triangle's box is smaller)
        assert tri[key] == quad[key], key
    assert [k for k, (off, _) in tri["lds_tables"].items() if off is not None] == [k for k, (off, _) in quad["lds_tables"].items() if off is not None]


# ---- tie guard ----
def _mesh_leaves(verts, faces):
    def build(s):
        return s.TriangleMesh(verts, faces, s.Lambertian((0.5, 0.5, 0.5)), return_triangles=True)[1]
    return build


def test_a_flat_lattice_keeps_its_library_tree():
    assert has_library_tree(scene_with(_mesh_leaves(*lattice(8, 0.37))))
    assert has_library_tree(scene_with(_mesh_leaves(*lattice(8, 0.37, y=1.3))))
    assert has_library_tree(scene_with(_mesh_leaves(*lattice(8, 0.5, y=1.25)))), "every normal and offset bit-equal: one plane for certain"


def test_a_lattice_of_8192_triangles_commits_and_keeps_its_library_tree():
    verts, faces = lattice(64, 0.37)
    assert faces.shape[0] == 8192
    s = rt.Scene()
    tris = s.TriangleMesh(verts, faces, s.Lambertian((0.5, 0.5, 0.5)), return_triangles=True)[1]
    s.SetWorld(s.BvhNode(tris))
    s.Camera((0.31, 3.7, 4.9), (0.5, 0, 0.5), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    t0 = time.perf_counter()
    s.Commit()
    print(f"commit of the 8192-triangle lattice: {time.perf_counter() - t0:.3f} s")
    assert has_library_tree(s) and s.info()["n_triangles"] == 8192


def _pair(first, second, filler=True):
    """Two faces as world leaves of their own, among a few spheres that make the world large enough for a tree."""
    def build(s):
        a, b = s.Lambertian((0.8, 0.2, 0.2)), s.Lambertian((0.2, 0.2, 0.8))
        items = [getattr(s, first[0])(*first[1:], a), getattr(s, second[0])(*second[1:], b)]
        return items + [s.Sphere((5.0 + k, 1.0, 0.3 * k), 0.3, a) for k in range(4)]
    return build


def test_coplanar_faces_tie_only_where_they_share_area():
    share = _pair(("Triangle", (0, 0, 0), (2, 0, 0), (0, 0, 2)), ("Triangle", (0.5, 0, 0.25), (2, 0, 0), (0, 0, 2)))
    assert not has_library_tree(scene_with(share)), "two coplanar triangles that overlap"
    inside = _pair(("Quad", (0, 0, 0), (4, 0, 0), (0, 0, 4)), ("Triangle", (1, 0, 1), (1, 0, 0), (0, 0, 1)))
    assert not has_library_tree(scene_with(inside)), "a triangle inside a coplanar quad"
    edge = _pair(("Quad", (0, 0, 0), (4, 0, 0), (0, 0, 4)), ("Triangle", (4, 0, 1), (2, 0, 0), (0, 0, 2)))
    assert has_library_tree(scene_with(edge)), "a triangle that meets a quad along one edge"
    vertex = _pair(("Triangle", (0, 0, 0), (2, 0, 0), (0, 0, 2)), ("Triangle", (2, 0, 0), (2, 0, 0), (2, 0, -2)))
    assert has_library_tree(scene_with(vertex)), "two triangles that meet in one vertex"
    halves = _pair(("Triangle", (0, 0, 0), (2, 0, 0), (0, 0, 2)), ("Triangle", (2, 0, 2), (-2, 0, 0), (0, 0, -2)))
    assert has_library_tree(scene_with(halves)), "the two halves of a square: one shared edge"
    apart = _pair(("Triangle", (0, 0, 0), (2, 0, 0), (0, 0, 2)), ("Triangle", (1.25, 0, 1.25), (2, 0, 0), (0, 0, 2)))
    assert has_library_tree(scene_with(apart)), "boxes that meet, triangles that do not"
    quads = _pair(("Quad", (0, 0, 0), (2, 0, 0), (0, 0, 2)), ("Quad", (2, 0, 0), (2, 0, 0), (0, 0, 2)))
    assert not has_library_tree(scene_with(quads)), "two quads keep the rule of the boxes that meet"


def test_a_transformed_pair_stays_conservative():
    def build(overlap):
        def inner(s):
            a, b = s.Lambertian((0.8, 0.2, 0.2)), s.Lambertian((0.2, 0.2, 0.8))
            moved = s.Translate(s.Triangle((0, 0, 0), (2, 0, 0), (0, 0, 2), b), (0.5 if overlap else 7.0, 0.0, 0.25))
            return [s.Triangle((0, 0, 0), (2, 0, 0), (0, 0, 2), a), moved] + [s.Sphere((5.0 + k, 1.0, 9.0), 0.3, a) for k in range(4)]
        return inner
    # (with a composite leaf the library's tree is the segmented walk's; the guard decides on it in the same way)
    assert scene_with(build(True)).dump_fast_nodes()[0].shape[0] == 0
    assert scene_with(build(False)).dump_fast_nodes()[0].shape[0] > 0


# ---- OBJ ----
OBJ = """# a square pyramid
o pyramid
v 0 0 0
v 1.5 0 0   # trailing comment
v 1.5 0 2.25 1.0
v 0 0 2.25
vn 0 1 0
vt 0.5 0.5
v +0.75 1.125e0 1.125
s off
f 1 2 5
f 2/1 3/1 5/1
f 3/1/1 4/1/1 5/1/1
f 4//1 1//1 5//1
f -5 -2 -3 -4
usemtl stone
"""


def test_obj_positions_and_faces(tmp_path):
    path = tmp_path / "pyramid.obj"
    path.write_text(OBJ)
    verts, faces = rt.load_obj(path)
    assert verts.dtype == np.float64 and faces.dtype == np.int32
    assert np.array_equal(verts, [[0, 0, 0], [1.5, 0, 0], [1.5, 0, 2.25], [0, 0, 2.25], [0.75, 1.125, 1.125]])
    assert np.array_equal(faces, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 3, 2], [0, 2, 1]])
    s = rt.Scene()
    assert s.TriangleMesh(verts, faces, s.Lambertian((0.5, 0.5, 0.5))) > 0


@pytest.mark.parametrize("text", ["v 0 0 0\nv 1 0 0\nv 0 1 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -99999999999999999999999\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 99999999999999999999999\n",
                                  "v 0,5 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n"],
                         ids=["no face", "index past the end", "relative index past the start", "index 0", "short vertex", "short face",
                              "index below every integer", "index above every integer", "decimal comma"])
def test_malformed_obj_files_are_invalid(tmp_path, text):
    path = tmp_path / "bad.obj"
    path.write_text(text)
    v, f, nv, nf = _lib.D3(), C.POINTER(C.c_int32)(), C.c_int(), C.c_int()
    assert rt.lib().rt_obj_load(str(path).encode(), C.byref(v), C.byref(nv), C.byref(f), C.byref(nf)) == RT_ERR_INVALID
    assert not v and not f, "nothing to free after a refusal"
    with pytest.raises(rt.RtowError):
        rt.load_obj(path)


def test_an_unreadable_obj_file_is_invalid(tmp_path):
    v, f, nv, nf = _lib.D3(), C.POINTER(C.c_int32)(), C.c_int(), C.c_int()
    assert rt.lib().rt_obj_load(str(tmp_path / "missing.obj").encode(), C.byref(v), C.byref(nv), C.byref(f), C.byref(nf)) == RT_ERR_INVALID
