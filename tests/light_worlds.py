"""Worlds of the light sampling tests (tests/test_lights_host.py, tests/test_lights_gpu.py): each builder returns the committed scene
and what the tests need to know about it.  ``emission`` is the table tests/light_restated.py evaluates textures from:
{material row: ("solid", rgb) | ("checker", inv_scale, even, odd)}; a material's row is its handle - 1."""
import math

import numpy as np

import raytracinginoneweekendincuda_amd as rt
from triangle_meshes import icosphere

QUAD, TRIANGLE, SPHERE, MSPHERE = 0, 1, 2, 3


def _camera(s):
    s.Camera((0, 0, 10), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0, background=(0, 0, 0))


def _lamps(s):
    """Three emissive materials: white, a checker of two colours, and a coloured one; (handles, emission table)."""
    white = s.DiffuseLight((4.0, 4.0, 4.0))
    checker = s.DiffuseLight(s.CheckerTexture(0.5, s.SolidColor((2.0, 1.0, 0.5)), s.SolidColor((0.5, 1.0, 2.0))))
    coloured = s.DiffuseLight((1.0, 2.0, 3.0))
    emission = {white - 1: ("solid", (4.0, 4.0, 4.0)), checker - 1: ("checker", 2.0, (2.0, 1.0, 0.5), (0.5, 1.0, 2.0)),
                coloured - 1: ("solid", (1.0, 2.0, 3.0))}
    return (white, checker, coloured), emission


def rotate_y_translate(p, degrees, offset, point):
    """A point or vector of an object under Translate(RotateY(object, degrees), offset) in world space, as the library's host code
    computes it: one IEEE operation at a time."""
    radians = degrees * 3.1415926535897932385 / 180.0
    sn, cs = math.sin(radians), math.cos(radians)
    x, y, z = (float(c) for c in p)
    out = [(cs * x) + (sn * z), y, (-sn * x) + (cs * z)]
    if point:
        out = [out[k] + float(offset[k]) for k in range(3)]
    return np.array(out, dtype=np.float64)


def mixed_world():
    """Every kind of light, an instance chain, a medium (excluded) and a BvhNode of emissive and plain leaves inside a list.
    Returns (scene, expected, emission): ``expected`` = the light table's rows in order as (kind, leaf, material row, dict of the
    geometry fields that must match bit for bit)."""
    s = rt.Scene()
    (white, checker, coloured), emission = _lamps(s)
    grey = s.Lambertian((0.5, 0.5, 0.5))
    expected = []
    top = []

    def leaf(handle):
        top.append(handle)
        return len(top) - 1

    k = leaf(s.Quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), white))
    expected.append((QUAD, k, white - 1, dict(a=(-1, 2, -1), b=(2, 0, 0), c=(0, 0, 2), s=4.0)))
    leaf(s.Sphere((0, -100, 0), 98.0, grey))
    k = leaf(s.Triangle((3, 1, 0), (1, 0, 0.5), (0, 1, 0.25), checker))
    area = 0.5 * float(np.sqrt(np.sum(np.cross((1, 0, 0.5), (0, 1, 0.25)) ** 2)))
    expected.append((TRIANGLE, k, checker - 1, dict(a=(3, 1, 0), b=(1, 0, 0.5), c=(0, 1, 0.25))))
    k = leaf(s.Sphere((-3, 1, 0), 0.5, white))
    expected.append((SPHERE, k, white - 1, dict(a=(-3, 1, 0), s=0.5)))
    k = leaf(s.MovingSphere((0, -1.5, 0), (0.5, -1.5, 0.25), 0.0, 1.0, 0.4, coloured))
    expected.append((MSPHERE, k, coloured - 1, dict(a=(0, -1.5, 0), b=(0.5, 0.0, 0.25), c=(0.0, 1.0, 0.0), s=0.4)))
    k = leaf(s.MakeBox((5, 0, 0), (6, 1, 2), white))
    for q, u, v in (((5, 0, 2), (1, 0, 0), (0, 1, 0)), ((6, 0, 2), (0, 0, -2), (0, 1, 0)), ((6, 0, 0), (-1, 0, 0), (0, 1, 0)),
                    ((5, 0, 0), (0, 0, 2), (0, 1, 0)), ((5, 1, 2), (1, 0, 0), (0, 0, -2)), ((5, 0, 0), (1, 0, 0), (0, 0, 2))):
        expected.append((QUAD, k, white - 1, dict(a=q, b=u, c=v)))
    q, u, v = (0, 0, 0.5), (1, 0, 0), (0, 1, 0)
    k = leaf(s.Translate(s.RotateY(s.Quad(q, u, v, coloured), 30.0), (1, 2, 3)))
    expected.append((QUAD, k, coloured - 1, dict(a=rotate_y_translate(q, 30.0, (1, 2, 3), True), b=rotate_y_translate(u, 30.0, (1, 2, 3), False),
                                                  c=rotate_y_translate(v, 30.0, (1, 2, 3), False),
                                                  n=rotate_y_translate((0, 0, 1), 30.0, (1, 2, 3), False), s=1.0)))
    leaf(s.ConstantMedium(s.Sphere((0, 5, 0), 1.0, white), 0.1, (1, 1, 1)))   # an emissive boundary: not a light
    members = {"plain sphere": s.Sphere((-6, 0, 0), 0.5, grey), "lamp sphere": s.Sphere((-6, 2, 0), 0.25, coloured),
               "plain quad": s.Quad((-7, 0, 2), (1, 0, 0), (0, 1, 0), grey), "lamp triangle": s.Triangle((-8, 0, 1), (1, 0, 0), (0, 1, 0), checker)}
    items = list(members.values())
    node = s.BvhNode(items)   # (sorts ``items`` as the reference sorts them: the order of the table below this leaf)
    k = leaf(s.HittableList([node]))
    for h in items:
        if h == members["lamp sphere"]:
            expected.append((SPHERE, k, coloured - 1, dict(a=(-6, 2, 0), s=0.25)))
        if h == members["lamp triangle"]:
            expected.append((TRIANGLE, k, checker - 1, dict(a=(-8, 0, 1), b=(1, 0, 0), c=(0, 1, 0), s=0.5)))
    s.SetWorld(s.HittableList(top))
    _camera(s)
    s.Commit()
    assert abs(area - 0.5 * math.sqrt(0.25 + 0.0625 + 1.0)) < 1e-15
    return s, expected, emission


def single_kind_world(kind):
    """Two lights of one kind (so that the selection matters) and a plain floor."""
    s = rt.Scene()
    (white, checker, coloured), emission = _lamps(s)
    floor = s.Quad((-10, -1, -10), (20, 0, 0), (0, 0, 20), s.Lambertian((0.5, 0.5, 0.5)))
    if kind == QUAD:
        lamps = [s.Quad((-1, 2, -1), (2, 0, 0), (0, 0, 2), checker), s.Quad((2, 1, -1), (0, 1.5, 0), (0.5, 0, 1), white)]
    elif kind == TRIANGLE:
        lamps = [s.Triangle((-1, 2, -1), (2, 0, 0.25), (0, 0.5, 2), checker), s.Triangle((2, 1, -1), (0, 1.5, 0), (0.5, 0, 1), coloured)]
    elif kind == SPHERE:
        lamps = [s.Sphere((-1, 2, 0), 0.5, checker), s.Sphere((2, 1.5, -1), 0.25, white)]
    else:
        lamps = [s.MovingSphere((-1, 2, 0), (-0.5, 2.25, 0.5), 0.0, 1.0, 0.5, coloured), s.MovingSphere((2, 1.5, -1), (2, 1.0, -1), 0.25, 0.75, 0.25, checker)]
    s.SetWorld(s.HittableList([floor] + lamps))
    _camera(s)
    s.Commit()
    return s, emission


def many_lights_world(n_lights):
    """``n_lights`` lights: the first n_lights - 6 faces of a level-2 icosphere of radius 2 about (0, 3, 0) as an emissive mesh, and six
    emissive quads beside it."""
    s = rt.Scene()
    (white, checker, coloured), emission = _lamps(s)
    verts, faces = icosphere(2, 2.0)
    assert 6 < n_lights <= len(faces) + 6
    mesh = s.TriangleMesh(verts + np.array([0.0, 3.0, 0.0]), faces[: n_lights - 6], checker)
    quads = [s.Quad((4 + 0.75 * k, 1, -1), (0.5, 0, 0), (0, 0.25 * (k + 1), 0.5), white if k % 2 else coloured) for k in range(6)]
    s.SetWorld(s.HittableList([mesh] + quads))
    _camera(s)
    s.Commit()
    return s, emission


def no_lights_world():
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    _camera(s)
    s.Commit()
    return s


def free_points(count, seed=7):
    """Points in free space below and beside the lamps of the worlds above, normals and material kinds to go with them, times."""
    g = np.random.default_rng(seed)
    points = np.ascontiguousarray(g.uniform((-2.0, -0.75, -2.0), (2.5, 0.5, 2.0), size=(count, 3)))
    normals = g.normal(size=(count, 3))
    normals = np.ascontiguousarray(normals / np.linalg.norm(normals, axis=1, keepdims=True))
    materials = np.ascontiguousarray(g.choice(np.array([0, 0, 0, 4, 1, 2, 3], dtype=np.uint8), size=count))
    times = np.ascontiguousarray(g.uniform(0.0, 1.0, size=count))
    return points, normals, materials, times
