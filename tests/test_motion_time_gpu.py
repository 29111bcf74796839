"""Moving spheres at ray times outside their own [time0, time1], on the GPU.

Every search of the world in another order than the reference's tree -- the library's SAH tree (kernel kind 64), the scan of
all leaves of a small BVH world (kind 8), RT_FLAG_ACCELERATE_LISTS, a sub-BVH over a group inside an instance, the segmented
walk of media worlds (kind bit 256), the thin-wave scan -- finds the reference's closest hit only while every hit lies inside
its leaf's box.  A camera whose shutter reaches outside a moving sphere's interval breaks that (tests/test_motion_time.py
pins it with the oracle), and then only the reference's order gives the reference's frame.  Each world here is built once
and rendered on a grid of motion x shutter pairs: the strict build equals the oracle, the kernel that must run runs, and
the kernels of the other column give the same frame bit for bit.
"""
import numpy as np
import pytest

from conftest import build_both
from frame_helpers import compare
from test_custom_scenes_gpu import _deep_media_world
from test_motion_time import H, SPP, W, field, instanced_group

pytestmark = pytest.mark.gpu

FLAG_FORCE_GENERAL, FLAG_ALWAYS_WALK, FLAG_REFERENCE_TREE, FLAG_ACCELERATE_LISTS = 2, 32, 128, 512

# id: (motion (time0, time1), shutter (time0, time1), rise of the moving spheres, every hit inside its box)
CASES = {
    "inside": ((0.0, 1.0), (0.0, 1.0), 0.6, True),
    "inside-half": ((0.0, 1.0), (0.25, 0.75), 0.6, True),
    "inside-instant": ((0.0, 1.0), (0.0, 0.0), 0.6, True),
    "non-unit": ((2.0, 5.0), (2.0, 5.0), 0.6, True),
    "reversed": ((1.0, 0.0), (0.0, 1.0), 0.6, True),
    "beyond-late": ((0.0, 1.0), (0.0, 3.0), 0.6, False),
    "beyond-both": ((0.25, 0.75), (0.0, 1.0), 0.6, False),
    "beyond-early": ((0.0, 1.0), (-1.0, 2.0), 0.6, False),
    "zero-interval": ((0.5, 0.5), (0.0, 1.0), 0.6, True),   # centre inf / NaN at every time: never hit
    "not-moving": ((0.0, 1.0), (0.0, 3.0), 0.0, True),      # c0 == c1: inside its box at every time
}
IDS = list(CASES)


def strict_equals_oracle(prod, orc, min_exact=0.99, fast_within=0.995, **kw):
    """The strict build against the oracle (the floors of test_custom_scenes_gpu.check); the fast build within 1e-5 on
    `fast_within` of the pixels (None: not compared).  Returns the strict frame and its stats."""
    want, stats = orc.render(W, H, SPP, want_stats=True)
    got, st = prod.render(W, H, SPP, variant=0, **kw)
    exact, within, worst = compare(got, want)
    print(f"kernel kind {st.kernel_kind}: bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
    assert st.rays == stats["rays"], "ray counter differs from the oracle's RayColor iterations"
    assert within >= 0.999 and exact >= min_exact
    fast, _ = prod.render(W, H, SPP, variant=1, **kw)
    assert np.isfinite(fast).all()
    if fast_within is not None:
        assert compare(fast, want)[1] >= fast_within
    return got, st


def same_frame(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case", IDS)
def test_bvh_world_of_spheres_and_quads(case):
    """(a) The library's tree where every hit stays in its box, the reference's tree otherwise -- same frame as the
    reference's tree walked on request (RT_FLAG_REFERENCE_TREE)."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(field("bvh", motion, shutter, rise=rise, moving_every=3, quads=True))
    got, st = strict_equals_oracle(prod, orc)
    assert st.kernel_kind == (64 if inside else 0)
    ref, st_ref = prod.render(W, H, SPP, variant=0, flags=FLAG_REFERENCE_TREE)
    assert st_ref.kernel_kind == 0 and st_ref.rays == st.rays
    assert same_frame(got, ref)


@pytest.mark.parametrize("case", IDS)
def test_bvh_world_of_spheres_thin_wave_scan(case):
    """(b) Spheres and moving spheres only: a wave with few live lanes may scan all leaves instead of walking
    (scan_grouped_ms, forced on with coop_threshold 65).  It must not where hits may leave their boxes."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(field("bvh", motion, shutter, rise=rise, moving_every=2))
    got, st = strict_equals_oracle(prod, orc)
    assert st.kernel_kind == (64 if inside else 0)
    walk, st_walk = prod.render(W, H, SPP, variant=0, coop_threshold=1)
    scan, st_scan = prod.render(W, H, SPP, variant=0, coop_threshold=65)
    assert st_walk.rays == st_scan.rays == st.rays
    assert same_frame(walk, scan) and same_frame(walk, got)


@pytest.mark.parametrize("case", IDS)
def test_small_bvh_world_scan(case):
    """(c) Twelve leaves: scanned in leaf order (kind 8) where every hit stays in its box, walked otherwise -- the frame of
    the walk on request (RT_FLAG_ALWAYS_WALK)."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(field("bvh", motion, shutter, rise=rise, n=11))
    got, st = strict_equals_oracle(prod, orc)
    assert st.kernel_kind == (8 if inside else 0)
    walk, st_walk = prod.render(W, H, SPP, variant=0, flags=FLAG_ALWAYS_WALK)
    assert st_walk.kernel_kind == (64 if inside else 0) and st_walk.rays == st.rays
    assert same_frame(got, walk)


@pytest.mark.parametrize("case", IDS)
def test_list_world_of_spheres_and_quads(case):
    """(d) The list world of (a): scanned in list order; through the library's tree on request (RT_FLAG_ACCELERATE_LISTS)
    only where every hit stays in its box; the leaves of a ray dealt to 4 and to 64 lanes -- one frame throughout."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(field("list", motion, shutter, rise=rise, moving_every=3, quads=True))
    got, st = strict_equals_oracle(prod, orc)
    assert st.kernel_kind == 8
    accel, st_accel = prod.render(W, H, SPP, variant=0, flags=FLAG_ACCELERATE_LISTS)
    assert st_accel.kernel_kind == (64 if inside else 8) and st_accel.rays == st.rays
    assert same_frame(got, accel)
    for ppw in (16, 1):
        grouped, stg = prod.render(W, H, SPP, variant=0, pixels_per_wave=ppw)
        assert stg.kernel_kind == 8 + 128 and stg.rays == st.rays
        assert same_frame(got, grouped), ppw


@pytest.mark.parametrize("world", ["bvh", "list"])
@pytest.mark.parametrize("case", IDS)
def test_instanced_group_of_moving_spheres(case, world):
    """(e) Translate(RotateY(HittableList(20 moving spheres))) over a floor: the group is scanned in list order, as the
    reference's HittableList is, not searched through a sub-BVH of the library's own."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(instanced_group(world, motion, shutter, rise=rise))
    strict_equals_oracle(prod, orc)


@pytest.mark.parametrize("case", [c for c in IDS if CASES[c][2] != 0.0])   # (its moving sphere always moves)
def test_deep_media_world_segmented_walk(case):
    """(f) A deep world with media and a moving sphere among its surface leaves: the segmented walk over the library's tree
    where every hit stays in its box, the reference's tree otherwise -- in both builds the frame of RT_FLAG_REFERENCE_TREE.
    As in test_custom_scenes_gpu's test of this world, the exact-pixel floor is 0.98 and the fast build is held to the
    reference-order walk of the same build rather than to the oracle: a contracted multiply-add sends a ray through a medium
    on another path in about 1 % of the pixels, with the shutter inside or beyond."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(_deep_media_world(("mist", "ball", "crate"), motion=motion, shutter=shutter))
    strict_equals_oracle(prod, orc, min_exact=0.98, fast_within=None, flags=FLAG_FORCE_GENERAL)
    for variant in (0, 1):
        got, st = prod.render(W, H, SPP, variant=variant, flags=FLAG_FORCE_GENERAL)
        ref, st_ref = prod.render(W, H, SPP, variant=variant, flags=FLAG_FORCE_GENERAL | FLAG_REFERENCE_TREE)
        assert bool(st.kernel_kind & 256) == inside, st.kernel_kind
        assert not (st_ref.kernel_kind & 256) and st_ref.rays == st.rays
        assert same_frame(got, ref), variant


def _media_and_trees(motion, shutter, rise):
    t0, t1 = motion

    def build(s, Rng):
        white, red = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05))
        fog = s.ConstantMedium(s.MovingSphere((-1.6, 0.0, 0.0), (-1.6, rise, 0.0), t0, t1, 0.9, white), 1.4, (0.2, 0.4, 0.9))
        # a list of composites inside an instance: the general-nesting interpreter (REF_TREE)
        members = [s.MovingSphere((0.0, -0.4, 0.0), (0.0, -0.4 + rise, 0.0), t0, t1, 0.5, s.Metal((0.8, 0.8, 0.8), 0.05)),
                   s.ConstantMedium(s.Sphere((1.0, -0.5, 0.3), 0.45, white), 2.0, (0.9, 0.6, 0.2)),
                   s.MakeBox((-0.3, -1.0, -0.9), (0.4, -0.2, -0.3), red)]
        group = s.Translate(s.RotateY(s.HittableList(members), 20.0), (1.2, 0.0, -0.4))
        balls = [s.MovingSphere((-3.0 + 1.2 * k, -0.6, 1.4), (-3.0 + 1.2 * k, -0.6 + rise, 1.4), t0, t1, 0.35,
                                (white, red)[k % 2]) for k in range(6)]
        floor = s.Quad((-30, -1, -30), (60, 0, 0), (0, 0, 60), s.Lambertian((0.4, 0.5, 0.3)))
        s.SetWorld(s.BvhNode([fog, group, floor] + balls))
        s.Camera((0, 1.2, 6.5), (0, 0.2, 0), (0, 1, 0), 50.0, W / H, 0.0, 10.0, shutter[0], shutter[1], (0.55, 0.65, 0.9))
        s.Commit()
    return build


@pytest.mark.parametrize("case", IDS)
def test_moving_medium_boundary_and_moving_sphere_in_a_tree(case):
    """(g) A ConstantMedium whose boundary is a moving sphere, and a moving sphere inside a general-nesting tree: kernels
    that walk the reference's tree in its order already (exact-pixel floor of the general-nesting tests)."""
    motion, shutter, rise, inside = CASES[case]
    prod, orc = build_both(_media_and_trees(motion, shutter, rise))
    strict_equals_oracle(prod, orc, min_exact=0.97)


def test_camera_change_after_commit_is_decided_per_launch():
    """Commit with the shutter inside the spheres' interval and render (library tree); then give the scene a camera whose
    shutter reaches beyond it, without a new commit: the next frame is the oracle's for that camera and that of a scene
    built with it from the start."""
    prod, _ = build_both(field("bvh", (0.0, 1.0), (0.0, 1.0), moving_every=3, quads=True))
    _, st_first = prod.render(W, H, SPP, variant=0)
    assert st_first.kernel_kind == 64
    prod.Camera((10.0, 3.0, 8.0), (0.0, 1.0, -1.0), (0, 1, 0), 30.0, W / H, 0.0, 10.0, 0.0, 3.0)
    fresh, orc = build_both(field("bvh", (0.0, 1.0), (0.0, 3.0), moving_every=3, quads=True))
    got, st = strict_equals_oracle(prod, orc)
    assert st.kernel_kind == 0
    again, st_again = fresh.render(W, H, SPP, variant=0)
    assert st_again.rays == st.rays and same_frame(got, again)
    # and back: the library's tree again
    prod.Camera((10.0, 3.0, 8.0), (0.0, 1.0, -1.0), (0, 1, 0), 30.0, W / H, 0.0, 10.0, 0.0, 1.0)
    _, st_back = prod.render(W, H, SPP, variant=0)
    assert st_back.kernel_kind == 64
