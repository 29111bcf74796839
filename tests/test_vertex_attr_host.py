"""Corner normals and texture coordinates of triangles and meshes on the host: what creation refuses (and that a refusal adds
nothing), emissive triangles, what commit reports, that scenes without attributes commit to what they committed to before, and
the OBJ reader's vn / vt.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib
from frame_helpers import render_params
from triangle_meshes import icosphere, lattice

W, H = 32, 24
Q, U, V = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
UP = np.array([[0.0, 0.0, 1.0]] * 3)
TC = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])


def commit(s, world):
    s.SetWorld(world)
    s.Camera((0.31, 3.7, 4.9), (0.5, 0, 0.5), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


def next_handle(s, m):
    """Hittable handles count up by one: the next one tells how many hittables the scene holds."""
    return s.Triangle(Q, U, V, m)


# ---- refusals ----
def test_a_refused_triangle_or_mesh_adds_nothing():
    s = rt.Scene()
    m, light = s.Lambertian((0.5, 0.5, 0.5)), s.DiffuseLight((4.0, 4.0, 4.0))
    verts, faces = icosphere(0, 1.0)
    first = next_handle(s, m)

    def bad(normals=None, texcoords=None, material=m):
        with pytest.raises(rt.RtowError):
            s.Triangle(Q, U, V, material, normals=normals, texcoords=texcoords)

    for value in (np.nan, np.inf):
        n = UP.copy()
        n[1, 2] = value
        bad(normals=n)
        t = TC.copy()
        t[2, 0] = value
        bad(texcoords=t)
    zero = UP.copy()
    zero[2] = 0.0
    bad(normals=zero)
    bad(normals=np.ones((3, 2)))            # a wrong shape
    bad(normals=np.ones(9))
    bad(texcoords=np.ones((3, 3)))
    bad(texcoords=TC, material=light)       # an emissive triangle takes no texture coordinates
    bad(normals=UP, texcoords=TC, material=light)
    bad(normals=UP, material=99)

    def bad_mesh(material=m, **kw):
        with pytest.raises(rt.RtowError):
            s.TriangleMesh(verts, faces, material, **kw)

    radial = verts.copy()
    tex = np.random.default_rng(1).uniform(size=(12, 2))
    spoiled = radial.copy()
    spoiled[11] = 0.0                        # the LAST vertex: every earlier triangle would have been acceptable
    bad_mesh(normals=spoiled)
    spoiled[11] = (np.nan, 0.0, 1.0)
    bad_mesh(normals=spoiled)
    spoiled_t = tex.copy()
    spoiled_t[11, 1] = np.nan
    bad_mesh(texcoords=spoiled_t)
    high = faces.copy()
    high[19, 2] = 12
    bad_mesh(normals=radial, normal_faces=high)          # an index at n_normals
    bad_mesh(normals=radial[:11])                        # ... through `faces` itself
    low = faces.copy()
    low[0, 0] = -1
    bad_mesh(texcoords=tex, texcoord_faces=low)
    bad_mesh(normals=radial, texcoords=tex[:5], texcoord_faces=faces)
    bad_mesh(normals=radial.ravel())                     # wrong shapes
    bad_mesh(normals=radial, normal_faces=faces[:19])
    bad_mesh(texcoords=np.ones((12, 3)))
    bad_mesh(normal_faces=faces)                         # indices without values
    bad_mesh(texcoords=tex, material=light)
    bad_mesh(normals=radial, texcoords=tex, material=light)
    assert next_handle(s, m) == first + 1, "a refused call added a hittable"

    # the C entry points themselves: 0 and a message
    L = rt.lib()
    v3 = lambda a: (C.c_double * 3)(*a)
    nan9 = (C.c_double * 9)(*([0.0] * 8 + [np.nan]))
    assert L.rt_triangle_attr(s._p, v3(Q), v3(U), v3(V), nan9, None, m) == 0 and b"normal" in L.rt_last_error()
    assert L.rt_triangle_attr(s._p, v3(Q), v3(U), v3(V), None, TC.ctypes.data_as(_lib.D3), light) == 0 and b"emissive" in L.rt_last_error()
    assert L.rt_triangle_attr(s._p, None, v3(U), v3(V), UP.ctypes.data_as(_lib.D3), None, m) == 0
    assert next_handle(s, m) == first + 2


def test_an_emissive_triangle_with_normals_is_a_light_like_its_flat_twin():
    def lights(attributed):
        s = rt.Scene()
        light, grey = s.DiffuseLight((4.0, 3.0, 2.0)), s.Lambertian((0.5, 0.5, 0.5))
        verts, faces = icosphere(0, 0.5)
        kw = dict(normals=verts / 0.5) if attributed else {}
        items = [s.Translate(s.RotateY(s.TriangleMesh(verts, faces, light, **kw), 20.0), (0.5, 2.0, 0.5)),
                 s.Triangle((0, 0, 0), (1, 0, 0), (0, 0, 1), light, **(dict(normals=[(0, 1, 0), (0.1, 1, 0), (0, 1, 0.1)]) if attributed else {})),
                 s.Quad((0, -1, 0), (1, 0, 0), (0, 0, 1), grey)]
        commit(s, s.HittableList(items))
        return s.lights(), s.info()

    (flat, flat_info), (smooth, smooth_info) = lights(False), lights(True)
    assert flat_info["n_lights"] == smooth_info["n_lights"] == 21
    assert flat_info["n_attributed_triangles"] == 0 and smooth_info["n_attributed_triangles"] == 21
    assert sorted(flat) == sorted(smooth)
    for name in flat:
        assert np.array_equal(flat[name], smooth[name]), name


# ---- what commit reports ----
def test_n_attributed_triangles_counts_the_rows_that_carry_attributes():
    verts, faces = lattice(3)
    tex = np.random.default_rng(2).uniform(size=(len(verts), 2))
    s = rt.Scene()
    m = s.Lambertian((0.5, 0.5, 0.5))
    items = [s.TriangleMesh(verts, faces, m),                                                     # 18 plain
             s.TriangleMesh(verts + (0, 1, 0), faces, m, normals=[(0, 1, 0), (0, 1, 0.5)], normal_faces=faces % 2),   # 18 with normals
             s.TriangleMesh(verts + (0, 2, 0), faces, m, texcoords=tex),                          # 18 with texture coordinates
             s.Translate(s.TriangleMesh(verts, faces[:5], m, normals=[(0, 1, 0)], normal_faces=faces[:5] * 0, texcoords=tex), (0, 3, 0)),
             s.Triangle(Q, U, V, m, normals=UP), s.Triangle(Q, U, V, m, texcoords=TC), s.Triangle(Q, U, V, m, normals=None, texcoords=None),
             s.Quad((5, 0, 0), (1, 0, 0), (0, 1, 0), m)]
    for world in (s.HittableList(items), s.BvhNode(list(items))):
        info = commit(s, world).info()
        assert info["n_triangles"] == 18 * 3 + 5 + 3 and info["n_quads"] == info["n_triangles"] + 1
        assert info["n_attributed_triangles"] == 18 + 18 + 5 + 2
    assert C.sizeof(_lib.SceneInfo) == 18 * 4, "rt_scene_info keeps its size"


def _plans(s):
    return [s.plan_launch(render_params(400, 300, 16, variant=variant, flags=flags), num_cus=256, adaptive=adaptive)
            for variant in (0, 1) for flags in (0, rt.FLAG_REFERENCE_TREE, rt.FLAG_FORCE_GENERAL) for adaptive in (False, True)]


def test_scenes_without_attributes_commit_to_what_they_committed_to():
    """The built-in scenes 0-12 carry no attribute row; a mesh given ``normals=None, texcoords=None`` is the mesh of the plain call
    (rt_triangle_mesh_attr with NULL arrays is rt_triangle_mesh): same info, same leaves, same nodes, same launch plans.  Scene 13
    is scene 12 in everything the search and the launcher see."""
    for scene_id in range(13):
        for world in (0, 1):
            assert rt.builtin_scene(scene_id, world, W, H).info()["n_attributed_triangles"] == 0, scene_id

    def mesh_scene(**kw):
        s = rt.Scene()
        verts, faces = icosphere(1, 1.5)
        lat, lat_faces = lattice(3, 2.0, -1.5)
        items = [s.Translate(s.TriangleMesh(verts, faces, s.Metal((0.8, 0.8, 0.8), 0.0), **kw), (0.5, 0.2, 0.5)),
                 s.TriangleMesh(lat - (2, 0, 2), lat_faces, s.Lambertian((0.5, 0.5, 0.5)), **kw), s.Triangle(Q, U, V, s.Dielectric(1.5), **kw)]
        return commit(s, s.BvhNode(items))

    plain, none = mesh_scene(), mesh_scene(normals=None, texcoords=None)
    assert plain.info() == none.info() and _plans(plain) == _plans(none)
    for a, b in zip(plain.dump_leaves() + plain.dump_nodes(), none.dump_leaves() + none.dump_nodes()):
        assert np.array_equal(a, b)

    for world in (0, 1):
        twelve, thirteen = rt.builtin_scene(12, world, 400, 400), rt.builtin_scene(13, world, 400, 400)
        a, b = twelve.info(), thirteen.info()
        assert b.pop("n_attributed_triangles") == 340 and a.pop("n_attributed_triangles") == 0 and a == b
        assert _plans(twelve) == _plans(thirteen)
        for x, y in zip(twelve.dump_leaves() + twelve.dump_nodes(), thirteen.dump_leaves() + thirteen.dump_nodes()):
            assert np.array_equal(x, y)


# ---- the OBJ reader ----
CUBE_CORNER = """# three faces of a cube corner, every corner form
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
v 1 0 1
vn 0 0 -1
vn 0 -1 0
vt 0 0
vt 1 0 0.5
vt 1 1
vt 0 +1
f 1/1/1 2/2/1 3/3/1 4/4/1      # a fanned quad, i/j/k
vn 1 0 0
f -6/-4/-2 -5/-3/2 6/3/-2       # negative indices, each relative to its own kind
f 1/1/3 5/4/3 6/2/3
"""


def test_obj_reader_returns_normals_and_texture_coordinates(tmp_path):
    path = tmp_path / "corner.obj"
    path.write_text(CUBE_CORNER)
    mesh = rt.load_obj(path, attributes=True)
    assert mesh._fields == ("vertices", "faces", "normals", "normal_faces", "texcoords", "texcoord_faces")
    assert mesh.vertices.shape == (6, 3) and mesh.normals.shape == (3, 3) and mesh.texcoords.shape == (4, 2)
    assert np.array_equal(mesh.normals, [(0, 0, -1), (0, -1, 0), (1, 0, 0)])
    assert np.array_equal(mesh.texcoords, [(0, 0), (1, 0), (1, 1), (0, 1)])
    assert np.array_equal(mesh.faces, [(0, 1, 2), (0, 2, 3), (0, 1, 5), (0, 4, 5)]) and mesh.faces.dtype == np.int32
    assert np.array_equal(mesh.texcoord_faces, [(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 3, 1)])
    assert np.array_equal(mesh.normal_faces, [(0, 0, 0), (0, 0, 0), (1, 1, 1), (2, 2, 2)])
    # without `attributes` the call returns what it returned: positions and faces
    plain = rt.load_obj(path)
    assert isinstance(plain, tuple) and len(plain) == 2
    assert np.array_equal(plain[0], mesh.vertices) and np.array_equal(plain[1], mesh.faces)
    # ... and the tuple goes into a mesh as it is
    s = rt.Scene()
    root = s.TriangleMesh(mesh.vertices, mesh.faces, s.Lambertian((0.5, 0.5, 0.5)), normals=mesh.normals, normal_faces=mesh.normal_faces,
                          texcoords=mesh.texcoords, texcoord_faces=mesh.texcoord_faces)
    assert commit(s, root).info()["n_attributed_triangles"] == 4


@pytest.mark.parametrize("faces,has_n,has_t", [("f 1 2 3\nf 1 3 4\n", False, False), ("f 1/1 2/2 3/3\nf 1/1 3/3 4/4\n", False, True),
                                                ("f 1//1 2//1 3//1\nf 1//1 3//1 4//1\n", True, False),
                                                ("f 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3 4/4/1\n", False, True),   # one corner lacks vn
                                                ("f 1/1/1 2/2/1 3/3/1\nf 1/1/1 3//1 4/4/1\n", True, False),  # one corner lacks vt
                                                ("f 1/1/1 2/2/1 3/3/1 4/4/1\n", True, True)])
def test_obj_reader_returns_a_kind_only_if_every_corner_names_it(tmp_path, faces, has_n, has_t):
    path = tmp_path / "square.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n" + faces)
    mesh = rt.load_obj(path, attributes=True)
    assert np.array_equal(mesh.faces, [(0, 1, 2), (0, 2, 3)])
    assert (mesh.normals is not None) == has_n and (mesh.normal_faces is not None) == has_n
    assert (mesh.texcoords is not None) == has_t and (mesh.texcoord_faces is not None) == has_t
    if has_n:
        assert np.array_equal(mesh.normals, [(0, 0, 1)]) and np.array_equal(mesh.normal_faces, np.zeros((2, 3)))
    if has_t:
        assert np.array_equal(mesh.texcoord_faces, mesh.faces) and mesh.texcoords.shape == (4, 2)


@pytest.mark.parametrize("text,line", [("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.5\nf 1 2 3\n", 4),                   # a vt with one number
                                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 1\nf 1 2 3\n", 4),
                                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/-2 3/1\n", 5),            # relative index before the first vt
                                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//0 3//1\n", 5),        # 0 is no index
                                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//-2 3//1\n", 5),
                                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/x 2/1 3/1\n", 5)])
def test_obj_reader_rejects_bad_attributes_with_file_and_line(tmp_path, text, line):
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(rt.RtowError) as e:
        rt.load_obj(path, attributes=True)
    assert f"bad.obj:{line}:" in str(e.value) and "status 1" in str(e.value)


def test_obj_reader_rejects_an_attribute_index_beyond_the_file(tmp_path):
    path = tmp_path / "beyond.obj"
    for text, what in (("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//2 3//1\n", "normal index out of range"),
                       ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/5\n", "texture coordinate index out of range")):
        path.write_text(text)
        with pytest.raises(rt.RtowError) as e:
            rt.load_obj(path, attributes=True)
        assert "beyond.obj" in str(e.value) and what in str(e.value)
    # the plain reader never reads j and k: the same files load
    assert rt.load_obj(path)[1].shape == (1, 3)
