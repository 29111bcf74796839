"""Moving spheres at ray times outside their own [time0, time1] -- CPU side (the oracle and the host flattener).

R/MovingSphere.h:51 computes frac = (t - time0) / (time1 - time0) without a clamp, while the sphere's box covers only
center0 .. center1.  A camera whose shutter reaches outside a sphere's interval therefore puts hits outside their leaf's box,
and the reference's BVH culls some of them -- which ones depends on the tree's shape and visiting order.  With the shutter
inside every interval the reference's frame does not depend on its tree.  These tests pin both halves of that premise with
the oracle alone (so that tests/test_motion_time_gpu.py cannot pass vacuously), and the host side of the library's answer:
no sub-BVH of its own over a group that holds a moving sphere.  The scene builders are shared with the GPU module.
"""
import numpy as np
import pytest

from conftest import OracleRng, OracleScene

W, H, SPP = 64, 32, 4

# (motion (time0, time1) of the moving spheres, camera shutter (time0, time1))
INSIDE = [((0.0, 1.0), (0.0, 1.0)), ((2.0, 5.0), (2.0, 5.0)), ((1.0, 0.0), (0.0, 1.0)), ((0.0, 1.0), (0.0, 0.0)),
          ((0.0, 1.0), (0.25, 0.75))]
BEYOND = [((0.0, 1.0), (0.0, 3.0)), ((0.25, 0.75), (0.0, 1.0)), ((0.0, 0.5), (0.0, 1.0)), ((0.0, 1.0), (-1.0, 2.0))]


def field(world, motion, shutter, rise=0.6, n=60, moving_every=1, quads=False):
    """A ground sphere and `n` spheres of radius 0.3 - 0.7 on a jittered grid; every `moving_every`-th of them is a moving
    sphere that rises by `rise` between time0 and time1 (the others are static), optionally two quads behind them.
    `world` is "bvh" (BvhNode world) or "list" (HittableList world)."""
    t0, t1 = motion

    def build(s, Rng):
        rnd = np.random.default_rng(2024)
        mats = [s.Lambertian((0.8, 0.3, 0.2)), s.Lambertian((0.2, 0.5, 0.8)), s.Metal((0.8, 0.8, 0.7), 0.1),
                s.Dielectric(1.5), s.Lambertian((0.3, 0.7, 0.3))]
        items = [s.Sphere((0.0, -1000.0, 0.0), 1000.0, s.Lambertian((0.5, 0.5, 0.5)))]
        for k in range(n):
            x = -7.0 + 14.0 * (k % 10) / 9.0 + float(rnd.uniform(-0.3, 0.3))
            z = -6.0 + 12.0 * (k // 10) / 5.0 + float(rnd.uniform(-0.3, 0.3))
            r = float(rnd.uniform(0.3, 0.7))
            y = r + float(rnd.uniform(0.0, 0.8))
            mat = mats[k % len(mats)]
            if k % moving_every == 0:
                items.append(s.MovingSphere((x, y, z), (x, y + rise, z), t0, t1, r, mat))
            else:
                items.append(s.Sphere((x, y, z), r, mat))
        if quads:
            items.append(s.Quad((-8.0, 0.0, -8.0), (16.0, 0.0, 0.0), (0.0, 5.0, 0.0), s.Metal((0.9, 0.9, 0.9), 0.05)))
            items.append(s.Quad((-8.0, 0.0, -8.0), (0.0, 0.0, 14.0), (0.0, 4.0, 0.0), s.Lambertian((0.8, 0.2, 0.2))))
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((10.0, 3.0, 8.0), (0.0, 1.0, -1.0), (0, 1, 0), 30.0, W / H, 0.0, 10.0, shutter[0], shutter[1])
        s.Commit()
    return build


def instanced_group(world, motion, shutter, moving=True, rise=0.6):
    """Translate(RotateY(HittableList(20 spheres))) over a floor quad: the group the flattener would give a sub-BVH of its own
    (flat_scene.h kSubBvhMinPrims).  `moving`: the twenty are moving spheres (rising by `rise`), else static spheres."""
    t0, t1 = motion

    def build(s, Rng):
        rnd = np.random.default_rng(77)
        mats = [s.Lambertian((0.8, 0.4, 0.2)), s.Metal((0.8, 0.8, 0.9), 0.0), s.Dielectric(1.5), s.Lambertian((0.2, 0.3, 0.8))]
        members = []
        for k in range(20):
            c = (float(rnd.uniform(-2.0, 2.0)), float(rnd.uniform(0.3, 1.6)), float(rnd.uniform(-1.5, 1.5)))
            r = float(rnd.uniform(0.25, 0.5))
            if moving:
                members.append(s.MovingSphere(c, (c[0], c[1] + rise, c[2]), t0, t1, r, mats[k % 4]))
            else:
                members.append(s.Sphere(c, r, mats[k % 4]))
        group = s.Translate(s.RotateY(s.HittableList(members), 25.0), (0.3, 0.0, -0.5))
        floor = s.Quad((-20.0, 0.0, -20.0), (40.0, 0.0, 0.0), (0.0, 0.0, 40.0), s.Lambertian((0.5, 0.6, 0.4)))
        items = [group, floor]
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((6.0, 3.0, 7.0), (0.0, 1.0, -0.5), (0, 1, 0), 40.0, W / H, 0.0, 10.0, shutter[0], shutter[1])
        s.Commit()
    return build


def oracle_frame(build, w=W, h=H, spp=SPP, want_stats=False):
    orc = OracleScene()
    build(orc, OracleRng)
    return orc.render(w, h, spp, want_stats=want_stats)


def same_pixels(a, b):
    return float(np.mean(np.all(a.view(np.uint64) == b.view(np.uint64), axis=-1)))


# ---- the premise, with the oracle alone ----
@pytest.mark.parametrize("motion,shutter", INSIDE)
def test_reference_frame_does_not_depend_on_the_tree_with_the_shutter_inside(motion, shutter):
    """Every ray time inside the spheres' interval: every hit lies in its leaf's box, and the reference's BVH world renders
    the frame of its list world bit for bit, with the same ray count."""
    bvh, st_bvh = oracle_frame(field("bvh", motion, shutter), want_stats=True)
    lst, st_lst = oracle_frame(field("list", motion, shutter), want_stats=True)
    assert st_bvh["rays"] == st_lst["rays"]
    assert np.array_equal(bvh.view(np.uint64), lst.view(np.uint64))


@pytest.mark.parametrize("motion,shutter", BEYOND)
def test_reference_frame_depends_on_the_tree_with_the_shutter_beyond(motion, shutter):
    """Ray times outside the interval put hits outside their boxes: the BVH world culls some that the list world finds.  More
    than 1 % of the pixels differ -- the worlds of the GPU tests show what they are meant to show."""
    bvh = oracle_frame(field("bvh", motion, shutter))
    lst = oracle_frame(field("list", motion, shutter))
    share = same_pixels(bvh, lst)
    print(f"motion {motion} shutter {shutter}: {share:.4f} of the pixels equal")
    assert share < 0.99


def test_reference_frame_of_an_instanced_group_depends_on_its_tree_with_the_shutter_beyond():
    """The group inside an instance: HittableList and BvhNode over the same twenty moving spheres give one frame with the
    shutter inside their interval and two different frames with the shutter beyond it."""
    def build(inner_bvh, shutter):
        def b(s, Rng):
            rnd = np.random.default_rng(77)
            mat = s.Lambertian((0.8, 0.4, 0.2))
            members = []
            for k in range(20):
                c = (float(rnd.uniform(-2.0, 2.0)), float(rnd.uniform(0.3, 1.6)), float(rnd.uniform(-1.5, 1.5)))
                members.append(s.MovingSphere(c, (c[0], c[1] + 0.6, c[2]), 0.0, 1.0, float(rnd.uniform(0.25, 0.5)), mat))
            inner = s.BvhNode(members) if inner_bvh else s.HittableList(members)
            floor = s.Quad((-20.0, 0.0, -20.0), (40.0, 0.0, 0.0), (0.0, 0.0, 40.0), s.Lambertian((0.5, 0.6, 0.4)))
            s.SetWorld(s.HittableList([s.Translate(s.RotateY(inner, 25.0), (0.3, 0.0, -0.5)), floor]))
            s.Camera((6.0, 3.0, 7.0), (0.0, 1.0, -0.5), (0, 1, 0), 40.0, W / H, 0.0, 10.0, shutter[0], shutter[1])
        return b
    inside = [oracle_frame(build(t, (0.0, 1.0))) for t in (False, True)]
    assert np.array_equal(inside[0].view(np.uint64), inside[1].view(np.uint64))
    beyond = [oracle_frame(build(t, (0.0, 3.0))) for t in (False, True)]
    assert same_pixels(beyond[0], beyond[1]) < 0.99


# ---- host side: which groups get a tree of the library's own ----
def _product(build):
    import raytracinginoneweekendincuda_amd as rt
    s = rt.Scene()
    build(s, rt.Rng)
    return s


@pytest.mark.parametrize("world", ["list", "bvh"])
def test_no_sub_bvh_over_a_group_of_moving_spheres(world):
    """Commit does not know the shutter, so a group holding a moving sphere whose centre moves stays a list, scanned in the
    reference's order; the same group of static spheres still gets its sub-BVH."""
    moving = _product(instanced_group(world, (0.0, 1.0), (0.0, 1.0), moving=True)).info()
    static = _product(instanced_group(world, (0.0, 1.0), (0.0, 1.0), moving=False)).info()
    world_nodes = 0 if world == "list" else 1   # the BvhNode world over two leaves: one node
    assert moving["n_moving_spheres"] == 20 and moving["n_objects"] == 1
    assert moving["n_nodes"] == world_nodes
    assert static["n_nodes"] > world_nodes


def test_group_of_moving_spheres_that_do_not_move_keeps_its_sub_bvh():
    """center0 == center1: the sphere is inside its box at every time, so nothing stands against the group's own tree."""
    info = _product(instanced_group("list", (0.0, 1.0), (0.0, 3.0), moving=True, rise=0.0)).info()
    assert info["n_moving_spheres"] == 20 and info["n_nodes"] > 0


def test_coincident_primitives_still_get_no_library_tree():
    """The other condition of the library's own trees (two leaves that tie): unchanged."""
    def build(s, Rng):
        red, green = s.Lambertian((0.8, 0.1, 0.1)), s.Lambertian((0.1, 0.8, 0.1))
        items = [s.Sphere((-1.2, 0.5, 0), 0.5, red), s.Sphere((-1.2, 0.5, 0), 0.5, green)]
        for k in range(12):
            items.append(s.MovingSphere((-5.0 + 0.9 * k, 0.2, 2.0), (-5.0 + 0.9 * k, 0.5, 2.0), 0.0, 1.0, 0.2, (red, green)[k % 2]))
        s.SetWorld(s.BvhNode(items))
        s.Camera((0.5, 1.5, 6), (0.5, 0.5, 0), (0, 1, 0), 45.0, W / H, 0.0, 10.0, 0.0, 1.0)
        s.Commit()
    s = _product(build)
    assert s.dump_fast_nodes()[0].shape[0] == 0
    # a world of moving spheres without a tie gets one (the shutter is a matter of the launch)
    assert _product(field("bvh", (0.0, 1.0), (0.0, 3.0), n=12)).dump_fast_nodes()[0].shape[0] > 0
