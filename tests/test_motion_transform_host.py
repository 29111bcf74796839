"""Moving instances on the host (include/rtow.h rt_moving_transform): what creation stores and refuses, that equal keys commit to
what the static Transform commits to, the conservative tie guard, and that the swept box holds every pose.  No GPU needed."""
import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
import motion_restated as mr
from frame_helpers import render_params
from test_transform_host import affine, bits, committed, rotation, W, H
from test_triangles_host import has_library_tree, scene_with
from triangle_meshes import icosphere

washed = lambda m: np.asarray(m, dtype=np.float64) + 0.0   # no negative zeros in a key: L0 + s * 0 turns a -0 entry into +0


# ---- 1. creation ----
def test_every_refusal_adds_nothing_and_what_is_stored_is_the_stated_difference():
    def build(refusals):
        s = rt.Scene()
        grey, light = s.Lambertian((0.5, 0.5, 0.5)), s.DiffuseLight((4.0, 4.0, 4.0))
        ball, lamp = s.Sphere((0, 0, 0), 1.0, grey), s.Sphere((0, 3, 0), 0.5, light)
        quad_lamp = s.Quad((-1, 4, -1), (2, 0, 0), (0, 0, 2), light)
        triangle_lamp = s.Triangle((-1, 5, -1), (2, 0, 0), (0, 0, 2), light)
        group = s.HittableList([ball, s.BvhNode([quad_lamp, s.Quad((0, 0, 0), (1, 0, 0), (0, 1, 0), grey)])])
        fog = s.ConstantMedium(s.HittableList([s.Quad((0, 0, 0), (1, 0, 0), (0, 1, 0), light), s.Sphere((0, 0, 0), 1.0, light)]), 0.5, (1, 1, 1))
        ok0, ok1 = affine(np.diag((1.0, 2.0, 3.0)), (1, 1, 1)), affine(washed(rotation((0, 1, 0), 15.0)) @ np.diag((1.0, 2.0, 3.0)), (2, 1, 1))
        eye = affine(np.eye(3))
        if refusals:
            bad_matrices = [affine(np.zeros((3, 3))), affine([[1, 2, 3], [2, 4, 6], [0, 1, 0]]), affine(np.diag((1.0, np.nan, 1.0))),
                            affine(np.eye(3), (0, np.inf, 0)), affine(np.diag((1e200, 1e200, 1e200))), affine(np.diag((1e-200, 1.0, 1e-200))),
                            affine(np.diag((1e-310, 1e5, 1e5)))]   # whatever rt_transform refuses (tests/test_transform_host.py)
            bad = [(999, ok0, ok1, 0.0, 1.0), (0, ok0, ok1, 0.0, 1.0)]
            bad += [(ball, m, ok1, 0.0, 1.0) for m in bad_matrices] + [(ball, ok0, m, 0.0, 1.0) for m in bad_matrices]   # for either key
            bad += [(ball, ok0, ok1, t0, t1) for t0, t1 in ((np.nan, 1.0), (0.0, np.inf), (-np.inf, 0.0), (1.0, 1.0), (1.0, 0.5), (0.0, np.nan))]
            bad += [(ball, eye, affine(np.diag((-1.0, -1.0, 1.0))), 0.0, 1.0),    # a half turn about Z: det = (1 - 2s)^2
                    (ball, eye, affine(np.diag((-1.0, 1.0, 1.0))), 0.0, 1.0),     # a mirror reached through zero: det = 1 - 2s
                    (ball, affine(washed(rotation((1, 1, 0), 10.0))), affine(washed(rotation((1, 1, 0), 190.0))), 0.0, 1.0)]
            bad += [(x, ok0, ok1, 0.0, 1.0) for x in (lamp, quad_lamp, triangle_lamp, group, s.Translate(s.RotateY(group, 10.0), (1, 0, 0)),
                                                       s.Scale(quad_lamp, 2.0))]
            for obj, m0, m1, t0, t1 in bad:
                with pytest.raises(rt.RtowError):
                    s.MovingTransform(obj, m0, m1, t0, t1)
            for call in (lambda: s.MovingTranslate(lamp, (0, 0, 0), (1, 0, 0)), lambda: s.MovingTranslate(ball, (0, 0, 0), (1, np.nan, 0)),
                         lambda: s.MovingTranslate(ball, (0, 0, 0), (1, 0, 0), 2.0, 2.0), lambda: s.MovingTranslate(999, (0, 0, 0), (1, 0, 0)),
                         lambda: s.MovingTransform(ball, np.zeros((3, 3)), ok1), lambda: s.MovingTransform(ball, ok0, np.concatenate([ok1, [[0, 0, 0, 2]]]))):
                with pytest.raises(rt.RtowError):
                    call()
            dp = lambda m: np.ascontiguousarray(m).ctypes.data_as(rt._lib.C.POINTER(rt._lib.C.c_double))
            assert rt.lib().rt_moving_transform(s._p, ball, None, dp(ok1), 0.0, 1.0) == 0 and rt.lib().rt_moving_transform(s._p, ball, dp(ok0), None, 0.0, 1.0) == 0
            with pytest.raises(rt.RtowError):
                s.moving_transform_keys(ball)
            with pytest.raises(rt.RtowError):
                s.moving_transform_keys(s.Transform(ball, ok0))
        placed = s.MovingTransform(s.HittableList([ball, fog]), ok0, ok1, 0.25, 2.0)   # a lamp inside a medium boundary is accepted
        return committed(s, [placed, lamp, quad_lamp]), placed, (ok0, ok1)

    (plain, h0, _), (refused, h1, (ok0, ok1)) = build(False), build(True)
    assert h1 == h0 + 4, "only the RotateY, the Translate, the Scale and the Transform of the refusal cases took handles"
    assert plain.info() == refused.info()
    assert np.array_equal(plain.dump_leaves()[1], refused.dump_leaves()[1])
    assert plain.info()["n_lights"] == 2 and plain.info()["n_xforms"] >= 1
    L0, t0, dL, dt, time0, dtime = refused.moving_transform_keys(h1)
    assert np.array_equal(bits(L0), bits(ok0[:, :3])) and np.array_equal(bits(t0), bits(ok0[:, 3]))
    assert np.array_equal(bits(dL), bits(ok1[:, :3] - ok0[:, :3])) and np.array_equal(bits(dt), bits(ok1[:, 3] - ok0[:, 3]))
    assert time0 == 0.25 and dtime == 2.0 - 0.25 and np.abs(dL).max() > 0.1
    # MovingTranslate: the identity at both keys
    s = rt.Scene()
    h = s.MovingTranslate(s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5))), (0.1, 0.2, 0.3), (1.0, -2.0, 0.7), -1.0, 3.0)
    L0, t0, dL, dt, time0, dtime = s.moving_transform_keys(h)
    assert np.array_equal(L0, np.eye(3)) and not dL.any() and np.array_equal(bits(t0), bits((0.1, 0.2, 0.3)))
    assert np.array_equal(bits(dt), bits(np.array((1.0, -2.0, 0.7)) - np.array((0.1, 0.2, 0.3)))) and (time0, dtime) == (-1.0, 4.0)


def test_python_takes_3x4_and_4x4_for_either_key():
    s = rt.Scene()
    ball = s.Sphere((0, 0, 0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))
    m0, m1 = affine(np.diag((1.0, 2.0, 3.0)), (4, 5, 6)), affine(np.diag((1.5, 2.0, 2.5)), (4, 6, 6))
    full = lambda m: np.concatenate([m, [[0.0, 0.0, 0.0, 1.0]]])
    a, b = s.moving_transform_keys(s.MovingTransform(ball, m0, m1)), s.moving_transform_keys(s.MovingTransform(ball, full(m0).tolist(), full(m1)))
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert a[4:] == (0.0, 1.0), "the default keys are at times 0 and 1"


# ---- 2. equal keys ----
@pytest.mark.parametrize("name,L", [("rotation", rotation((1, -2, 0.5), 47.0)), ("non-uniform scale", np.diag((0.3, 7.0, 1.9))),
                                    ("shear", np.array([[1.0, 0.8, -0.4], [0.0, 1.0, 0.6], [0.0, 0.0, 1.0]])),
                                    ("mirror", rotation((0, 1, 1), 20.0) @ np.diag((-1.5, 1.0, 0.8)))])
def test_equal_keys_commit_to_what_the_static_transform_commits_to(name, L):
    m = affine(washed(L), (0.25, -3.0, 1e3))

    def build(moving):
        s = rt.Scene()
        grey = s.Lambertian((0.5, 0.5, 0.5))
        verts, faces = icosphere(1, 0.9)
        children = [s.Sphere((0.3, -0.2, 0.1), 0.8, grey), s.MakeBox((-0.5, -0.4, -0.6), (0.7, 0.5, 0.4), grey), s.TriangleMesh(verts, faces, grey),
                    s.ConstantMedium(s.MakeBox((-1, -1, -1), (1, 1, 1), grey), 0.5, (1, 1, 1))]
        place = (lambda x: s.MovingTransform(x, m, m, 0.5, 0.75)) if moving else (lambda x: s.Transform(x, m))
        items = [s.Translate(place(c), (3.0 * k, 0.0, 0.0)) for k, c in enumerate(children)]
        items.append(s.ConstantMedium(place(s.MakeBox((-1, 2, -1), (1, 3, 1), grey)), 0.5, (1, 1, 1)))   # the step as a medium's boundary
        return committed(s, items)

    a, b = build(True), build(False)
    assert a.info()["n_xforms"] == b.info()["n_xforms"] >= 9
    (ka, ba), (kb, bb) = a.dump_leaves(), b.dump_leaves()
    assert np.array_equal(ka, kb)
    # the stated widening: 16 eps of the largest coordinate among the sixteen corners, outward; a Translate above it adds half an ulp
    reach = np.abs(bb).max()
    slack = 17 * 2.0 ** -52 * reach
    lo, hi = slice(0, 6, 2), slice(1, 6, 2)
    assert (ba[:, lo] <= bb[:, lo]).all() and (ba[:, hi] >= bb[:, hi]).all(), "never tighter than the static box"
    assert np.abs(ba - bb).max() <= slack, (np.abs(ba - bb).max(), slack)
    for adaptive in (False, True):
        for variant in (0, 1):
            p = render_params(W, H, 4, variant=variant)
            assert a.plan_launch(p, adaptive=adaptive) == b.plan_launch(p, adaptive=adaptive)


# ---- 3. tie guard ----
def test_the_tie_guard_takes_a_face_under_a_moving_step_for_its_whole_swept_box():
    def build(overlap, moving=True):
        def inner(s):
            a, b = s.Lambertian((0.8, 0.2, 0.2)), s.Lambertian((0.2, 0.2, 0.8))
            # tests/test_transform_host.py's pair: a triangle in the plane y = 2 of object space, scaled into the world plane y = 1
            L, x = [[1.0, 0.0, 0.25], [0.0, 0.5, 0.0], [0.0, 0.0, 1.5]], 0.5 if overlap else 7.0
            child = s.Triangle((0, 2, 0), (2, 0, 0), (0, 0, 2), b)
            # key 0 stands 3 units above the other face, key 1 reaches it: only the swept box meets it
            moved = s.MovingTransform(child, affine(L, (x, 3.0, 0.25)), affine(L, (x, 0.0, 0.25))) if moving else s.Transform(child, affine(L, (x, 3.0, 0.25)))
            return [s.Triangle((0, 1, 0), (2, 0, 0), (0, 0, 2), a), moved] + [s.Sphere((5.0 + k, 1.0, 9.0), 0.3, a) for k in range(4)]
        return inner
    assert not has_library_tree(scene_with(build(True))), "the swept box reaches the other face"
    assert has_library_tree(scene_with(build(False))), "the same faces 7 units apart"
    assert has_library_tree(scene_with(build(True, moving=False))), "the static face at key 0 alone ties with nothing"


# ---- 4. box ----
import test_transform_gpu as tg   # noqa: E402  (its children and matrices; importing it runs nothing on a GPU)

SHEARED = np.diag((1.7, 0.6, 1.2)) @ tg.SHEAR
MOVING_CHAINS = {   # keys at times 0 and 1; the children are about 2 units across
    "shear and scale between two rotations": [("moving", (affine(washed(rotation((1, 2, -0.5), 27.0) @ SHEARED), (3.0, -1.5, 0.75)),
                                                         affine(washed(rotation((1, 2, -0.5), 47.0) @ SHEARED), (3.5, -1.0, 0.25)), 0.0, 1.0))],
    "mirror that travels": [("moving", (affine(np.diag((-1.3, 0.9, 1.1)), (-4.0, 0.5, 1.0)), affine(np.diag((-1.3, 0.9, 1.1)), (4.0, 0.5, 1.0)), 0.0, 1.0))],
    "translate moving rotate_y moving_translate": [("translate", (1.25, -0.5, 2.0)),
                                                   ("moving", (affine(washed(rotation((0.3, -1, 0.2), -63.0)) @ np.diag((0.8, 1.4, 1.1)), (0.5, 0.25, -1.0)),
                                                               affine(washed(rotation((0.3, -1, 0.2), -48.0)) @ np.diag((0.9, 1.2, 1.1)), (-0.5, 0.75, -1.0)), 0.0, 1.0)),
                                                   ("rotate_y", 28.0),
                                                   ("moving_translate", ((-0.3, 0.2, 0.1), (0.9, -0.4, 0.6), 0.0, 1.0))],
}


def child_and_its_points(s, name):
    """A child of tests/test_transform_gpu.py with the eight corners of its box and, for the mesh, its vertices."""
    child = tg.child_of(s, name)
    lo, hi = np.array(s.BoundingBox(child)).reshape(3, 2).T
    points = [np.array([(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]]) for i in range(2) for j in range(2) for k in range(2)]
    if name == "icosahedron":
        points += list(icosphere(0, tg.ICO_R)[0])
    return child, points


@pytest.mark.parametrize("chain_name", sorted(MOVING_CHAINS))
@pytest.mark.parametrize("name", tg.CHILDREN)
def test_the_leaf_box_holds_every_pose(name, chain_name):
    s = rt.Scene()
    child, points = child_and_its_points(s, name)
    handle, chain = mr.build_chain(s, child, MOVING_CHAINS[chain_name])
    committed(s, [handle])
    box = s.dump_leaves()[1][0].reshape(3, 2)
    assert np.array_equal(bits(box), bits(np.array(s.BoundingBox(handle)).reshape(3, 2))), "the leaf dump reports the swept box"
    rng = np.random.default_rng(32)
    sv = np.concatenate([[0.0, 1.0, -0.25, 1.25, -7.0, 9.0], rng.uniform(-0.25, 1.25, 1994)])   # keys at [0, 1]: s = clamp(tm)
    assert len(sv) == 2000 and ((sv < 0) | (sv > 1)).mean() > 0.2
    worst = -np.inf
    for p in points:
        moved = mr.forward_points(chain, np.broadcast_to(p, (len(sv), 3)), sv)
        worst = max(worst, (box[:, 0] - moved).max(), (moved - box[:, 1]).max())
    print(f"{name} under {chain_name}: the farthest point lies {-worst:.3g} inside the box")
    assert worst <= 0.0
