"""General affine instances on the host (include/rtow.h rt_transform): what creation stores and refuses, the bounding box, the
convenience constructors' matrices, the light rows and the tie guard under a Transform, and that a scene without one commits to
what it committed to.  No GPU needed."""
import math

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import transform_restated as tr
from frame_helpers import render_params
from test_triangles_host import has_library_tree, scene_with

W, H = 32, 24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotation(axis, degrees):
    a, (x, y, z) = np.radians(degrees), np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def affine(L, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(L, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


def committed(s, items):
    s.SetWorld(s.HittableList(items))
    s.Camera((0.0, 2.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


# ---- creation ----
def test_every_refusal_adds_nothing():
    def build(refusals):
        s = rt.Scene()
        grey, light = s.Lambertian((0.5, 0.5, 0.5)), s.DiffuseLight((4.0, 4.0, 4.0))
        ball, lamp = s.Sphere((0, 0, 0), 1.0, grey), s.Sphere((0, 3, 0), 0.5, light)
        moving_lamp = s.MovingSphere((2, 3, 0), (2, 3.5, 0), 0.0, 1.0, 0.25, light)
        group = s.HittableList([ball, s.BvhNode([lamp, s.Quad((0, 0, 0), (1, 0, 0), (0, 1, 0), grey)])])
        fog = s.ConstantMedium(s.Sphere((0, 0, 0), 1.0, light), 0.5, (1, 1, 1))   # an emissive sphere as a medium's boundary is no lamp
        ok = affine(np.diag((1.0, 2.0, 3.0)), (1, 1, 1))
        if refusals:
            bad = [(999, ok), (0, ok), (ball, affine(np.zeros((3, 3)))), (ball, affine([[1, 2, 3], [2, 4, 6], [0, 1, 0]])),
                   (ball, affine(np.diag((1.0, np.nan, 1.0)))), (ball, affine(np.eye(3), (0, np.inf, 0))),
                   (ball, affine(np.diag((1e200, 1e200, 1e200)))),     # the determinant overflows
                   (ball, affine(np.diag((1e-200, 1.0, 1e-200)))),     # the determinant underflows to zero
                   (ball, affine(np.diag((1e-310, 1e5, 1e5)))),         # a finite determinant, an inverse that overflows
                   (lamp, ok), (moving_lamp, ok), (group, ok), (s.Translate(s.RotateY(group, 10.0), (1, 0, 0)), ok)]
            for obj, m in bad:
                with pytest.raises(rt.RtowError):
                    s.Transform(obj, m)
            for call in (lambda: s.Scale(ball, (1.0, 0.0, 1.0)), lambda: s.Scale(lamp, 2.0), lambda: s.RotateX(lamp, 30.0), lambda: s.RotateZ(999, 30.0)):
                with pytest.raises(rt.RtowError):
                    call()
            assert rt.lib().rt_transform(s._p, ball, None) == 0
        placed = s.Transform(s.HittableList([ball, fog]), ok)
        return committed(s, [placed, lamp, moving_lamp]), placed

    (plain, h0), (refused, h1) = build(False), build(True)
    assert h1 == h0 + 2, "only the RotateY and the Translate that carried a refused child took handles"
    info0, info1 = plain.info(), refused.info()
    assert info0 == info1
    assert np.array_equal(plain.dump_leaves()[1], refused.dump_leaves()[1])
    assert info0["n_lights"] == 2 and info0["n_xforms"] >= 1


@pytest.mark.parametrize("name,L", [("rotation", rotation((1, -2, 0.5), 47.0)), ("non-uniform scale", np.diag((0.3, 7.0, 1.9))),
                                    ("shear", np.array([[1.0, 0.8, -0.4], [0.0, 1.0, 0.6], [0.0, 0.0, 1.0]])),
                                    ("mirror", rotation((0, 1, 1), 20.0) @ np.diag((-1.5, 1.0, 0.8)))])
def test_the_stored_inverse_is_the_inverse(name, L):
    s = rt.Scene()
    t = (0.25, -3.0, 1e3)
    h = s.Transform(s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5))), affine(L, t))
    gotL, gott, Li = s.transform_matrices(h)
    assert np.array_equal(bits(gotL), bits(L)) and np.array_equal(bits(gott), bits(t)), "stored as given"
    cond = np.linalg.cond(L)
    err = np.abs(gotL @ Li - np.eye(3)).max()
    print(f"{name}: cond {cond:.3f}, |L Li - I| {err:.3g} = {err / 2.0 ** -52:.2f} ulp")
    assert err <= 64 * 2.0 ** -52 * cond
    assert (np.linalg.det(L) < 0) == (name == "mirror")
    # ... and it is the cofactor formula of the header, operation for operation
    c = np.array([[L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1], L[1, 2] * L[2, 0] - L[1, 0] * L[2, 2], L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]],
                  [L[0, 2] * L[2, 1] - L[0, 1] * L[2, 2], L[0, 0] * L[2, 2] - L[0, 2] * L[2, 0], L[0, 1] * L[2, 0] - L[0, 0] * L[2, 1]],
                  [L[0, 1] * L[1, 2] - L[0, 2] * L[1, 1], L[0, 2] * L[1, 0] - L[0, 0] * L[1, 2], L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0]]])
    det = (L[0, 0] * c[0, 0] + L[0, 1] * c[0, 1]) + L[0, 2] * c[0, 2]
    assert np.array_equal(bits(Li), bits(c.T / det))


def test_the_bounding_box_is_that_of_the_eight_corners():
    s = rt.Scene()
    grey = s.Lambertian((0.5, 0.5, 0.5))
    for child in (s.Sphere((0.3, -0.2, 0.1), 0.8, grey), s.MakeBox((-0.5, -0.4, -0.6), (0.7, 0.5, 0.4), grey), s.Quad((0, 0, 0), (1, 0, 0), (0, 0, 1), grey)):
        h = s.Transform(child, affine(rotation((1, 2, 3), 33.0) @ np.diag((1.5, 0.5, 2.0)), (4.0, -1.0, 0.5)))
        lo, hi = np.array(s.BoundingBox(child)).reshape(3, 2).T
        corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in range(2) for j in range(2) for k in range(2)])
        moved = tr.forward_points([("transform", s.transform_matrices(h))], corners)
        want = np.stack([moved.min(axis=0), moved.max(axis=0)], axis=1)
        thin = want[:, 1] - want[:, 0] < 0.0001   # the corner constructor's padding (AABB.h:114-120)
        want[thin] += (-0.00005, 0.00005)
        assert np.array_equal(bits(np.array(s.BoundingBox(h)).reshape(3, 2)), bits(want))
    flat = s.Scale(s.Quad((0, 0, 0), (1, 0, 0), (0, 0, 1), grey), (2.0, 5.0, 2.0))   # the child's padded thin axis, scaled: wide enough now
    assert np.array_equal(bits(np.array(s.BoundingBox(flat)).reshape(3, 2)[1]), bits((5.0 * (0.0 - 0.00005), 5.0 * (0.0 + 0.00005))))


def test_the_convenience_constructors_fill_the_stated_entries():
    s = rt.Scene()
    ball = s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))
    for degrees in (30.0, -118.5, 90.0):
        radians = degrees * 3.1415926535897932385 / 180.0
        sn, cs = math.sin(radians), math.cos(radians)
        L, t, _ = s.transform_matrices(s.RotateX(ball, degrees))
        assert np.array_equal(bits(L), bits([[1, 0, 0], [0, cs, -sn], [0, sn, cs]])) and not t.any()
        L, t, _ = s.transform_matrices(s.RotateZ(ball, degrees))
        assert np.array_equal(bits(L), bits([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]])) and not t.any()
    L, t, Li = s.transform_matrices(s.Scale(ball, (2.0, -0.5, 4.0)))
    assert np.array_equal(L, np.diag((2.0, -0.5, 4.0))) and np.array_equal(Li, np.diag((0.5, -2.0, 0.25))) and not t.any()
    assert np.array_equal(s.transform_matrices(s.Scale(ball, 3.0))[0], np.diag((3.0, 3.0, 3.0)))
    # RotateX by +90 degrees takes +y to +z; RotateZ takes +x to +y
    assert np.allclose(s.transform_matrices(s.RotateX(ball, 90.0))[0] @ (0, 1, 0), (0, 0, 1), atol=1e-15)
    assert np.allclose(s.transform_matrices(s.RotateZ(ball, 90.0))[0] @ (1, 0, 0), (0, 1, 0), atol=1e-15)
    with pytest.raises(rt.RtowError):
        s.transform_matrices(ball)


def test_python_takes_3x4_and_4x4_and_refuses_a_bad_last_row():
    s = rt.Scene()
    ball = s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))
    m = affine(np.diag((1.0, 2.0, 3.0)), (4, 5, 6))
    full = np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    for a, b in zip(s.transform_matrices(s.Transform(ball, m)), s.transform_matrices(s.Transform(ball, full.tolist()))):
        assert np.array_equal(bits(a), bits(b))
    for last in ((0, 0, 0, 2), (0, 0, 1e-9, 1), (np.nan, 0, 0, 1)):
        with pytest.raises(rt.RtowError):
            s.Transform(ball, np.concatenate([m, [last]]))
    for shape in ((3, 3), (4, 3), (12,)):
        with pytest.raises(rt.RtowError):
            s.Transform(ball, np.zeros(shape))


# ---- lights ----
def test_light_rows_under_a_transform_are_the_restatement_and_s_is_the_transformed_area():
    s = rt.Scene()
    light, grey = s.DiffuseLight((5.0, 4.0, 3.0)), s.Lambertian((0.5, 0.5, 0.5))
    q, u, v = np.array((-1.0, 0.25, -1.0)), np.array((2.0, 0.0, 0.5)), np.array((0.25, 0.0, 2.0))
    steps = [("translate", (0.5, 3.0, -0.25)), ("transform", affine(rotation((1, 0, 0.3), 160.0) @ np.diag((1.5, 1.0, 0.6)), (0.1, 0.2, 0.3))),
             ("rotate_y", 40.0), ("transform", affine([[1.0, 0.3, 0.0], [0.0, 1.0, 0.0], [0.2, 0.0, -1.0]]))]
    quad, chain = tr.build_chain(s, s.Quad(q, u, v, light), steps)
    triangle, chain_t = tr.build_chain(s, s.HittableList([s.Triangle(q, u, v, light), s.Sphere((9, 9, 9), 0.1, grey)]), steps[1:2])
    rigid = s.Translate(s.RotateY(s.Quad(q, u, v, light), 40.0), (0, 1, 0))
    committed(s, [quad, triangle, rigid, s.Sphere((0, -100, 0), 99.0, grey)])
    L = s.lights()
    assert L["kind"].tolist() == [0, 1, 0] and L["leaf"].tolist() == [0, 1, 2], "an emissive quad or triangle under a Transform is listed"
    twin = rt.Scene()
    n0 = committed(twin, [twin.Quad(q, u, v, twin.DiffuseLight((5.0, 4.0, 3.0)))]).lights()["n"]   # the normal as constructed

    def area(b, c):   # |b x c| as the host forms it, one operation at a time
        x = np.array([b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]])
        return np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    for k, ch in ((0, chain), (1, chain_t)):
        a, b, c = tr.forward_points(ch, q[None])[0], tr.forward_vectors(ch, u[None])[0], tr.forward_vectors(ch, v[None])[0]
        assert np.array_equal(bits(L["a"][k]), bits(a)) and np.array_equal(bits(L["b"][k]), bits(b)) and np.array_equal(bits(L["c"][k]), bits(c))
        n = tr.forward_normals(ch, n0)[0]
        assert np.array_equal(bits(L["n"][k]), bits(n)), "the constructed normal through the restated rule"
        assert abs(np.sqrt(L["n"][k].dot(L["n"][k])) - 1.0) <= 4 * 2.0 ** -53
        assert abs(L["n"][k].dot(b)) < 1e-14 and abs(L["n"][k].dot(c)) < 1e-14, "still the normal of the transformed face"
        want = area(b, c) if k == 0 else 0.5 * area(b, c)
        assert L["s"][k] == want and abs(L["s"][k] / L["s"][2] - (1.0, 0.5)[k]) > 0.05, "the area of the transformed primitive"
    assert L["s"][2] == area(u, v), "without a Transform s is the constructed primitive's area"


# ---- nothing without a Transform moved ----
@pytest.mark.parametrize("scene_id", range(14))
def test_a_scene_without_a_transform_commits_to_what_it_committed_to(scene_id):
    """The built-ins 0 .. 13 hold no Transform: built while another scene of the process holds Transforms, committed or not, they
    dump the leaves, nodes, lights, info and launch plans of the scene built before any Transform call of this test."""
    for world_kind in (0, 1):
        plain = rt.builtin_scene(scene_id, world_kind, W, H)
        other = rt.Scene()
        ball = other.Sphere((0, 0, 0), 1.0, other.Lambertian((0.5, 0.5, 0.5)))
        committed(other, [other.Transform(other.Scale(other.RotateX(other.RotateZ(ball, 10.0), 20.0), 2.0), affine(np.eye(3), (1, 2, 3)))])
        s = rt.builtin_scene(scene_id, world_kind, W, H)
        assert plain.info() == s.info() and other.info()["n_xforms"] == 4
        assert np.array_equal(plain.dump_camera(), s.dump_camera())
        for dump in ("dump_leaves", "dump_nodes", "dump_fast_nodes"):
            for x, y in zip(getattr(plain, dump)(), getattr(s, dump)()):
                assert np.array_equal(x, y), dump
        La, Lb = plain.lights(), s.lights()
        for key in La:
            same_bits = lambda a: bits(a) if a.dtype == np.float64 else a
            assert np.array_equal(same_bits(La[key]), same_bits(Lb[key])), key
        for adaptive in (False, True):
            for variant in (0, 1):
                p = render_params(W, H, 4, variant=variant)
                assert plain.plan_launch(p, adaptive=adaptive) == s.plan_launch(p, adaptive=adaptive)


def test_scene_14_counts_a_transform_as_one_step():
    s = rt.builtin_scene(14, 1, W, H)
    info = s.info()
    # icosphere: 1; slab: Translate + RotateX; ellipsoid: Translate + Scale; fog: Translate + Scale
    assert info["n_xforms"] == 7 and info["n_media"] == 1 and info["n_attributed_triangles"] == 320 and info["n_lights"] == 1
    with pytest.raises(rt.RtowError):
        rt.builtin_scene(15, 0, W, H)


# ---- tie guard ----
def test_the_tie_guard_finds_a_coplanar_face_under_a_transform():
    def build(overlap):
        def inner(s):
            a, b = s.Lambertian((0.8, 0.2, 0.2)), s.Lambertian((0.2, 0.2, 0.8))
            # a triangle in the plane y = 2 of object space, scaled by 0.5 in y and sheared within the plane: world plane y = 1
            m = affine([[1.0, 0.0, 0.25], [0.0, 0.5, 0.0], [0.0, 0.0, 1.5]], (0.5 if overlap else 7.0, 0.0, 0.25))
            moved = s.Transform(s.Triangle((0, 2, 0), (2, 0, 0), (0, 0, 2), b), m)
            return [s.Triangle((0, 1, 0), (2, 0, 0), (0, 0, 2), a), moved] + [s.Sphere((5.0 + k, 1.0, 9.0), 0.3, a) for k in range(4)]
        return inner
    assert not has_library_tree(scene_with(build(True))), "two coplanar overlapping faces, one under a Transform"
    assert has_library_tree(scene_with(build(False))), "the same faces apart"
