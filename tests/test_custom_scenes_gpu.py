"""HIP megakernel against the CPU oracle on scenes built constructor by constructor on BOTH sides.

The built-in scenes (ids 0..11) are transcribed twice, once per side; the scenes here are written once, as a
function of a scene object, and run against raytracinginoneweekendincuda_amd.Scene (C-ABI, include/rtow.h) and
against conftest.OracleScene (oracle_c_* constructors of oracle/rtow_oracle.c).  They cover what no built-in scene
pins: the duplicated span-1 BVH leaf holding a ConstantMedium (SURVEY Q7, R/BvhNode.h:63-67 + R/ConstantMedium.h:52-94),
quads in every axis pairing / boxes thin, far and instanced, and the reference's general object nesting
(R/Instance.h:31-56,74-150, R/ConstantMedium.h:32-50, R/HittableList.h:21-57, R/BvhNode.h:50-90,124-143).
"""
import numpy as np
import pytest

from conftest import build_both
from frame_helpers import compare

pytestmark = pytest.mark.gpu

TOL = 1e-5
W, H, SPP = 64, 32, 4


def check(build, w=W, h=H, spp=SPP, min_exact=0.99, variants=(0, 1), min_within_fast=0.995):
    prod, orc = build_both(build)
    want, stats = orc.render(w, h, spp, want_stats=True)
    for variant in variants:
        got, st = prod.render(w, h, spp, variant=variant)
        exact, within, worst = compare(got, want, TOL)
        print(f"variant {variant}: kernel kind {st.kernel_kind}, bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
        assert np.isfinite(got).all()
        if variant == 0:
            assert st.rays == stats["rays"], "ray counter differs from the oracle's RayColor iterations"
            assert within >= 0.999 and exact >= min_exact
        else:
            assert within >= min_within_fast
    return want


# ---- Q7: the duplicated leaf of a span-1 BvhNode ----
def _one_medium(world):
    def build(s, Rng):
        ball = s.Sphere((0, 0, -3), 1.0, s.Dielectric(1.5))
        fog = s.ConstantMedium(ball, 0.8, (0.9, 0.2, 0.2))
        items = [fog]
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 60, W / H, 0.0, 10.0)
        s.Commit()
    return build


def test_span1_bvh_medium_leaf_is_hit_twice_like_the_oracle():
    """BvhNode over one ConstantMedium: left == right == the leaf, so the medium is queried twice per visit and draws
    twice (the second call with tMax = the first hit).  The oracle walks the pointer tree exactly like
    R/BvhNode.h:109-155; the kernel's threaded walk must consume the same draws."""
    bvh = check(_one_medium("bvh"), spp=8)
    lst = check(_one_medium("list"), spp=8)
    assert not np.array_equal(bvh, lst), "the duplicated leaf must show (the list world hits the medium once)"


def test_span1_medium_leaf_inside_a_larger_bvh():
    """Three leaves: the median split leaves one span-1 node (the box medium, sorted first on x) beside a span-2 node."""
    def build(s, Rng):
        white = s.Lambertian((0.73, 0.73, 0.73))
        smoke = s.ConstantMedium(s.MakeBox((-3.2, -1, -4), (-1.6, 0.8, -2.5), white), 0.9, (0.1, 0.1, 0.1))
        items = [s.Sphere((0.3, 0, -3), 0.8, s.Metal((0.8, 0.7, 0.6), 0.2)),
                 smoke,
                 s.Sphere((2.4, 0, -3.5), 0.9, s.Lambertian((0.2, 0.4, 0.8)))]
        s.SetWorld(s.BvhNode(items))
        s.Camera((0, 0.5, 2), (0, 0, -3), (0, 1, 0), 60, W / H, 0.0, 10.0)
        s.Commit()
    check(build, spp=8)


# ---- quads and boxes ----
def _quad_zoo(world_kind):
    def build(s, Rng):
        red, green, grey = s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15)), s.Lambertian((0.73, 0.73, 0.73))
        metal, glass, light = s.Metal((0.8, 0.8, 0.9), 0.1), s.Dielectric(1.5), s.DiffuseLight((4.0, 4.0, 4.0))
        items = []
        e = [(1.5, 0, 0), (0, 1.5, 0), (0, 0, 1.5)]
        k = 0
        for a in range(3):
            for p in range(3):
                if p == a:
                    continue
                q = 3 - a - p
                for su, sv in ((1, 1), (-1, 1), (1, -1)):
                    u = tuple(su * c for c in e[p])
                    v = tuple(sv * c for c in e[q])
                    org = [-6.0 + 1.7 * (k % 7), -2.0 + 1.9 * (k // 7), -3.0 - 0.3 * k]
                    items.append(s.Quad(org, u, v, (red, green, grey, metal)[k % 4]))
                    k += 1
        items.append(s.Quad((-1.0, 3.5, -4.0), (2.0, 0.3, 0.1), (0.2, 1.5, -0.4), green))          # not axis-aligned
        items.append(s.Quad((-8.0, 6.0, -12.0), (16.0, 0, 0), (0, 0, 14.0), light))
        items.append(s.MakeBox((-5.0, -3.0, -2.0), (-3.5, -1.0, -0.5), grey))                      # plain box leaf
        items.append(s.MakeBox((1000.0, -3.0, -2.0), (1001.5, -1.0, -0.5), red))                   # far from the origin
        items.append(s.MakeBox((0.0, -3.0, -2.0), (1.5, -3.0 + 1e-9, -0.5), green))                # paper-thin
        items.append(s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.6, 2.8, 1.6), glass), 18.0), (2.5, -3.0, -3.0)))
        items.append(s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.2, 1.2, 1.2), metal), -25.0), (-1.5, -3.0, -1.0)))
        items.append(s.Sphere((0.0, -1003.0, 0.0), 1000.0, grey))
        s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
        s.Camera((0.5, 1.0, 9.0), (0.0, 0.0, -2.0), (0, 1, 0), 55.0, 96 / 64, 0.0, 10.0, 0.0, 1.0, (0.1, 0.1, 0.15))
        s.Commit()
    return build


@pytest.mark.parametrize("world_kind", [0, 1])
def test_quad_zoo_matches_the_oracle(world_kind):
    """Every (normal axis, u axis) pairing and winding of an axis-aligned quad, a slanted quad, boxes plain / far /
    paper-thin / instanced: the AAQuad and BoxRec shortcuts of flat_scene.h against R/Quad.h:52-99 evaluated in full
    by the oracle (not against the kernel's own general test)."""
    check(_quad_zoo(world_kind), w=96, h=64, spp=8)


# ---- lanes-per-ray scan of list worlds (rt_render_params.pixels_per_wave, render.hip scan_leaves_grouped) ----
def _cornell(world_kind):
    """The Cornell box with its two instanced boxes (R/kernel.cu:363-398, config C4) through the shared constructor names."""
    def build(s, Rng):
        red, white, green = s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.12, 0.45, 0.15))
        light = s.DiffuseLight((15.0, 15.0, 15.0))
        items = [s.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green), s.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),
                 s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), light), s.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),
                 s.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white), s.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white),
                 s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (165, 330, 165), white), 15.0), (265, 0, 295)),
                 s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (165, 165, 165), white), -18.0), (130, 0, 65))]
        s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
        s.Camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0, (0, 0, 0))
        s.Commit()
    return build


def _spheres_and_quads(world_kind):
    """A list of 13 primitives (the list-of-primitives kernel): more leaves than lanes per ray at most group widths."""
    def build(s, Rng):
        items = [s.Sphere((0, -1000, 0), 1000.0, s.Lambertian((0.5, 0.5, 0.5)))]
        for k in range(9):
            mat = (s.Lambertian((0.2 + 0.08 * k, 0.3, 0.7 - 0.06 * k)), s.Metal((0.8, 0.7, 0.5), 0.05 * k), s.Dielectric(1.5))[k % 3]
            items.append(s.Sphere((-4.0 + k, 0.45 + 0.05 * k, -1.0 + 0.7 * (k % 4)), 0.45 + 0.05 * k, mat))
        items.append(s.Quad((-5, 0, -4), (10, 0, 0), (0, 4, 0), s.Metal((0.9, 0.9, 0.9), 0.0)))
        items.append(s.Quad((-5, 0, -4), (0, 0, 8), (0, 3, 0), s.Lambertian((0.8, 0.2, 0.2))))
        items.append(s.MovingSphere((2, 2, 0), (2, 2.4, 0), 0.0, 1.0, 0.4, s.Lambertian((0.1, 0.8, 0.2))))
        s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
        s.Camera((1, 2.5, 9), (0, 0.8, 0), (0, 1, 0), 40.0, W / H, 0.05, 9.0, 0.0, 1.0)
        s.Commit()
    return build


@pytest.mark.parametrize("name,world_kind", [("cornell", 0), ("cornell", 1), ("zoo", 1), ("prims", 0), ("prims", 1)])
def test_lanes_per_ray_list_scan_gives_the_one_lane_per_ray_frame(name, world_kind):
    """pixels_per_wave < 64: the leaves of every ray are dealt to 64 / pixels_per_wave lanes and one reduction per group picks
    the hit -- the same frame, ray count and (checked against the oracle once) RNG streams as the sequential scan, for every
    group width, in both builds.  Cornell as a BvhNode world is a small world rendered by the list kernels in leaf order."""
    build = {"cornell": _cornell, "zoo": _quad_zoo, "prims": _spheres_and_quads}[name](world_kind)
    prod, orc = build_both(build)
    w, h, spp = 48, 32, 6
    want = orc.render(w, h, spp)
    for variant in (0, 1):
        ref, st0 = prod.render(w, h, spp, variant=variant, pixels_per_wave=64)
        assert st0.kernel_kind in (8, 10) and st0.pixels_per_wave == 64
        if variant == 0:
            exact, within, _ = compare(ref, want, TOL)
            assert within >= 0.999 and exact >= 0.99
        for ppw in (32, 16, 8, 4, 2, 1):
            got, st = prod.render(w, h, spp, variant=variant, pixels_per_wave=ppw)
            assert st.kernel_kind == st0.kernel_kind + 128 and st.pixels_per_wave == ppw, (st.kernel_kind, st.pixels_per_wave)
            assert st.rays == st0.rays, (ppw, st.rays, st0.rays)
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (name, variant, ppw)


def test_pixels_per_wave_zero_means_one_lane_per_ray():
    """pixels_per_wave = 0 is the library's choice, and measured on every split of C4 that choice is one lane per ray (a grouped
    pass of a mixed list is longer than a plain one: DESIGN.md section 6), also for a film of a few thousand pixels."""
    prod, _ = build_both(_cornell(0))
    small, st_small = prod.render(64, 64, 4, variant=0, pixels_per_wave=0)
    assert st_small.pixels_per_wave == 64 and st_small.kernel_kind == 10
    ref, st_ref = prod.render(64, 64, 4, variant=0, pixels_per_wave=64)
    assert np.array_equal(small.view(np.uint64), ref.view(np.uint64)) and st_small.rays == st_ref.rays


# ---- coincident primitives: the order of the tests decides ----
def _coincident(world_kind):
    def build(s, Rng):
        red, green, blue, white = (s.Lambertian((0.8, 0.1, 0.1)), s.Lambertian((0.1, 0.8, 0.1)), s.Lambertian((0.1, 0.1, 0.8)),
                                   s.Lambertian((0.8, 0.8, 0.8)))
        mirror = s.Metal((0.9, 0.9, 0.9), 0.0)
        items = [s.Sphere((-1.2, 0.5, 0), 0.5, red), s.Sphere((-1.2, 0.5, 0), 0.5, green),             # the same sphere twice: first one wins
                 s.Quad((0.2, 0, -0.5), (1.2, 0, 0), (0, 1.2, 0), blue), s.Quad((0.6, 0.3, -0.5), (1.2, 0, 0), (0, 1.2, 0), red),  # one plane: the later one wins where they overlap
                 s.MakeBox((2.2, 0, -1), (3.0, 0.8, -0.2), green), s.Quad((2.0, 0.2, -0.2), (1.2, 0, 0), (0, 0.4, 0), mirror),   # a quad in the plane of a box face
                 s.Quad((-6, 0, -6), (12, 0, 0), (0, 0, 12), white)]
        for k in range(12):   # enough leaves for a BvhNode world to be walked rather than scanned
            items.append(s.Sphere((-5.0 + 0.9 * k, 0.2, 2.0), 0.2, (red, green, blue)[k % 3]))
        s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
        s.Camera((0.5, 1.5, 6), (0.5, 0.5, 0), (0, 1, 0), 45.0, W / H, 0.0, 10.0)
        s.Commit()
    return build


@pytest.mark.parametrize("world_kind", [0, 1])
def test_coincident_primitives_resolve_like_the_reference(world_kind):
    """Two identical spheres, two overlapping quads in one plane, a quad in the plane of a box face: a ray gets the same t
    from both and the ORDER of the tests decides (first sphere: R/Sphere.h:38,50 strict; last quad: R/Quad.h:59-64
    inclusive).  Such a world gets no library tree (its near-child-first order is not the reference's) -- it is walked /
    scanned in the reference's order and must equal the oracle; the lanes-per-ray scan resolves ties the same way.
    (The twin spheres and the coplanar quads trip the guard on their own, so the box face of this world never meets an
    out-of-order walk: that tie is exercised in tests/test_tie_worlds_gpu.py.)"""
    prod, orc = build_both(_coincident(world_kind))
    assert prod.dump_fast_nodes()[0].shape[0] == 0, "a world with coincident primitives must not get a library tree"
    want, stats = orc.render(W, H, 8, want_stats=True)
    got, st = prod.render(W, H, 8, variant=0)
    exact, within, worst = compare(got, want, TOL)
    print(f"coincident world {world_kind}: kernel kind {st.kernel_kind}, bit-exact {exact:.4f}, within {within:.4f}")
    assert st.rays == stats["rays"] and within >= 0.999 and exact >= 0.99
    accel, _ = prod.render(W, H, 8, variant=0, flags=512)   # RT_FLAG_ACCELERATE_LISTS has no tree to use
    assert np.array_equal(accel.view(np.uint64), got.view(np.uint64))
    if world_kind == 1:
        for ppw in (16, 4, 1):
            grouped, stg = prod.render(W, H, 8, variant=0, pixels_per_wave=ppw)
            assert stg.kernel_kind & 128 and stg.rays == st.rays
            assert np.array_equal(grouped.view(np.uint64), got.view(np.uint64)), ppw


# ---- the segmented walk of deep composite worlds with media (flat_scene.h FastOrder / SegMedium, render.hip seg_advance) ----
def _deep_media_world(media, motion=(0.0, 1.0), shutter=(0.0, 1.0)):
    """~110 leaves under one BvhNode: a field of plain boxes, spheres of every material, instanced boxes, an instanced cluster of
    40 spheres (sub-BVH + cooperative scan), and ConstantMedium leaves as `media` names them:
      mist    a sphere of radius 60 around everything, camera included (sorted first by the reference's build)
      ball    a small glass ball with fog inside, in the middle of the field
      crate   a rotated, translated box of smoke (boundary = six quads behind two transforms)
      far     a ball of fog behind the camera's far wall that hardly any ray's line meets
      lone    (extra leaves arranged so that one medium ends up alone in a span-1 node: hit twice)
    `motion`: (time0, time1) of its moving sphere; `shutter`: the camera's (time0, time1) (tests/test_motion_time_gpu.py)."""
    def build(s, Rng):
        rng = Rng(7)
        u = rng.uniform
        white, grey = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.4, 0.45, 0.4))
        items = []
        for i in range(8):
            for k in range(8):
                x0, z0, h = -8.0 + 2.0 * i, -8.0 + 2.0 * k, 0.2 + 1.1 * u()
                items.append(s.MakeBox((x0, -1.0, z0), (x0 + 1.9, -1.0 + h, z0 + 1.9), grey if (i + k) % 3 else white))
        mats = [s.Lambertian((0.7, 0.2, 0.2)), s.Metal((0.8, 0.8, 0.9), 0.1), s.Dielectric(1.5), s.DiffuseLight((3.0, 3.0, 2.5))]
        for k in range(16):
            items.append(s.Sphere((-7.0 + 0.95 * k, 0.8 + 0.6 * u(), -6.0 + 12.0 * u()), 0.3 + 0.25 * u(), mats[k % 4]))
        items.append(s.MovingSphere((3.0, 1.5, 1.0), (3.0, 2.0, 1.0), motion[0], motion[1], 0.5, mats[0]))
        items.append(s.Quad((-4.0, 6.0, -4.0), (8.0, 0, 0), (0, 0, 8.0), s.DiffuseLight((4.0, 4.0, 4.0))))
        for k in range(4):
            box = s.MakeBox((0, 0, 0), (0.9, 1.6 + 0.3 * k, 0.9), white)
            items.append(s.Translate(s.RotateY(box, 15.0 + 20.0 * k), (-5.0 + 3.0 * k, 0.4, 4.0 - 2.5 * k)))
        cluster = [s.Sphere((1.6 * u(), 1.6 * u(), 1.6 * u()), 0.12, white) for _ in range(40)]
        items.append(s.Translate(s.RotateY(s.HittableList(cluster), 15.0), (-1.0, 1.2, 3.0)))
        if "mist" in media:
            items.append(s.ConstantMedium(s.Sphere((0, 0, 0), 60.0, s.Dielectric(1.5)), 0.004, (1, 1, 1)))
        if "ball" in media:
            ball = s.Sphere((0.5, 1.4, 0.0), 1.0, s.Dielectric(1.5))
            items.append(ball)
            items.append(s.ConstantMedium(ball, 0.6, (0.2, 0.4, 0.9)))
        if "crate" in media:
            crate = s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.5, 1.5, 1.5), white), -18.0), (-4.0, 0.6, -1.0))
            items.append(s.ConstantMedium(crate, 0.9, (0.05, 0.05, 0.05)))
        if "far" in media:
            items.append(s.ConstantMedium(s.Sphere((30.0, 25.0, -40.0), 2.0, s.Dielectric(1.5)), 0.5, (0.9, 0.9, 0.1)))
        if "lone" in media:
            # the reference's median split puts a lone leaf into a span-1 node when a span of three is cut 1 + 2: three leaves far
            # out on +x, the medium first among them by its box's lower edge
            items.append(s.ConstantMedium(s.Sphere((40.0, 1.0, 0.0), 1.5, s.Dielectric(1.5)), 0.7, (0.9, 0.3, 0.3)))
            items.append(s.Sphere((44.0, 1.0, 0.0), 1.0, mats[1]))
            items.append(s.Sphere((47.0, 1.0, 0.0), 1.0, mats[0]))
        for extra in range(media.count("more")):   # more media than the segmented walk handles: the reference-order kernel takes over
            items.append(s.ConstantMedium(s.Sphere((-6.0 + 3.0 * extra, 3.0, -3.0), 0.5, s.Dielectric(1.5)), 0.8, (0.3, 0.9, 0.3)))
        s.SetWorld(s.BvhNode(items))
        s.Camera((12.0, 6.0, 14.0), (0.0, 0.5, 0.0), (0, 1, 0), 38.0, W / H, 0.05, 18.0, shutter[0], shutter[1], (0.35, 0.45, 0.7))
        s.Commit()
    return build


@pytest.mark.parametrize("media", [("mist",), ("ball",), ("mist", "ball", "crate"), ("mist", "ball", "crate", "far"), ("lone", "ball"), ()])
def test_segmented_walk_matches_the_oracle_and_the_reference_order_walk(media):
    """Deep composite worlds with media go through the library's tree, one walk per run of surface leaves between two media
    (kernel kind bit 256).  Only media draw random numbers, and each is tested with exactly the closest hit the reference has
    when it reaches it, so frame, ray count and RNG streams equal the oracle's (which walks the reference's pointer tree in
    the reference's order) and those of the kernel that walks the reference's tree (RT_FLAG_REFERENCE_TREE)."""
    prod, orc = build_both(_deep_media_world(media))
    want, stats = orc.render(W, H, 6, want_stats=True)
    for variant in (0, 1):
        seg, st = prod.render(W, H, 6, variant=variant, flags=2)            # RT_FLAG_FORCE_GENERAL: plain textures would pick a non-rich kernel
        ref, st_ref = prod.render(W, H, 6, variant=variant, flags=2 | 128)
        assert st.kernel_kind & 256, f"expected the segmented walk, got kernel kind {st.kernel_kind}"
        assert not (st_ref.kernel_kind & 256)
        assert st.rays == st_ref.rays
        assert np.array_equal(seg.view(np.uint64), ref.view(np.uint64)), (media, variant)
        if variant == 0:
            exact, within, worst = compare(seg, want, TOL)
            print(f"media {media}: kernel kind {st.kernel_kind}, bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
            assert st.rays == stats["rays"] and within >= 0.999 and exact >= 0.98


def test_more_media_than_the_segmented_walk_handles_fall_back():
    prod, orc = build_both(_deep_media_world(("mist", "ball", "crate", "far", "more", "more")))
    got, st = prod.render(W, H, 4, variant=0, flags=2)
    assert not (st.kernel_kind & 256)
    want = orc.render(W, H, 4)
    exact, within, _ = compare(got, want, TOL)
    assert within >= 0.999 and exact >= 0.98


def test_segmented_walk_continues_the_same_rng_streams():
    """Progressive rendering across the two walks: 3 + 5 samples with the saved per-pixel streams, one half by each kernel, equal
    8 samples by either -- the streams (media draws included) are consumed identically."""
    import raytracinginoneweekendincuda_amd as rt
    prod, _ = build_both(_deep_media_world(("mist", "ball", "crate")))
    one, _ = prod.render(W, H, 8, variant=0, flags=2)
    film = rt.Film(W, H)
    film.render(prod, 3, variant=0, flags=2 | rt.FLAG_ACCUMULATE)
    film.render(prod, 5, variant=0, flags=2 | 128 | rt.FLAG_ACCUMULATE | rt.FLAG_KEEP_RNG_STATE)
    assert np.array_equal(film.download().view(np.uint64), one.view(np.uint64))


# ---- general nesting (R/Instance.h, R/ConstantMedium.h, R/HittableList.h, R/BvhNode.h take any Hittable*) ----
def _room(s, items, cam_from=(0, 1.2, 6.5), cam_at=(0, 0.6, 0), vfov=50.0, bg=(0.55, 0.65, 0.9), world="bvh"):
    floor = s.Quad((-30, -1, -30), (60, 0, 0), (0, 0, 60), s.Lambertian(s.CheckerTexture(0.8, s.SolidColor((0.2, 0.3, 0.1)),
                                                                                         s.SolidColor((0.9, 0.9, 0.9)))))
    items = list(items) + [floor]
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera(cam_from, cam_at, (0, 1, 0), vfov, W / H, 0.0, 10.0, 0.0, 1.0, bg)
    s.Commit()


NESTINGS = {}


def nesting(fn):
    NESTINGS[fn.__name__] = fn
    return fn


@nesting
def medium_under_transforms(s, Rng):
    """Translate(RotateY(ConstantMedium(box))) -- the reference's scene 8 has the medium OUTSIDE the instance; here it is inside."""
    white = s.Lambertian((0.73, 0.73, 0.73))
    fog = s.ConstantMedium(s.MakeBox((0, 0, 0), (1.6, 2.0, 1.6), white), 1.1, (0.9, 0.9, 0.9))
    inst = s.Translate(s.RotateY(fog, 25.0), (-1.4, -1.0, -0.5))
    ball = s.ConstantMedium(s.Sphere((0, 0, 0), 0.9, white), 2.0, (0.1, 0.2, 0.7))
    inst2 = s.RotateY(s.Translate(ball, (1.7, 0.0, 0.4)), -40.0)
    _room(s, [inst, inst2])


@nesting
def medium_in_medium(s, Rng):
    """ConstantMedium whose boundary is a ConstantMedium (R/ConstantMedium.h:32: boundary is any Hittable*): the inner
    medium's stochastic hit is the outer one's boundary query, twice per call."""
    white = s.Lambertian((0.73, 0.73, 0.73))
    inner = s.ConstantMedium(s.Sphere((0, 0.3, 0), 1.3, white), 3.0, (0.8, 0.3, 0.3))
    outer = s.ConstantMedium(inner, 1.5, (0.2, 0.8, 0.3))
    _room(s, [outer, s.Sphere((2.6, 0, -1), 1.0, s.Metal((0.8, 0.8, 0.8), 0.0))])


@nesting
def instance_of_composites(s, Rng):
    """Translate(RotateY(HittableList[box, Translate(sphere), ConstantMedium(sphere)])): a list of non-primitives inside an instance."""
    white, red = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05))
    members = [s.MakeBox((-0.5, -1, -0.5), (0.5, 0.2, 0.5), white),
               s.Translate(s.Sphere((0, 0, 0), 0.45, s.Dielectric(1.5)), (0.0, 0.7, 0.0)),
               s.ConstantMedium(s.Sphere((1.3, -0.3, 0.2), 0.7, white), 2.5, (0.3, 0.3, 0.9)),
               s.RotateY(s.MakeBox((-1.9, -1, -0.4), (-1.1, 0.6, 0.4), red), 30.0)]
    group = s.Translate(s.RotateY(s.HittableList(members), 20.0), (0.2, 0.0, -0.8))
    _room(s, [group, s.Sphere((-2.9, 0.0, -1.5), 1.0, s.Metal((0.7, 0.6, 0.5), 0.1))])


@nesting
def bvh_inside_a_list_world(s, Rng):
    """HittableList world whose members include a BvhNode over primitives and a BvhNode over composites."""
    rng = Rng(7, 3)
    mats = [s.Lambertian((0.7, 0.3, 0.2)), s.Metal((0.8, 0.8, 0.9), 0.05), s.Dielectric(1.5), s.Lambertian((0.2, 0.5, 0.8))]
    balls = []
    for k in range(23):
        x, y, z = -4 + 8 * rng.uniform(), -0.7 + 1.5 * rng.uniform(), -3 + 4 * rng.uniform()
        balls.append(s.Sphere((x, y, z), 0.3, mats[k % 4]))
    comps = [s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (0.8, 1.4, 0.8), mats[0]), 15.0), (-3.2, -1.0, 1.2)),
             s.ConstantMedium(s.Sphere((2.6, 0.2, 1.4), 0.8, mats[0]), 1.5, (0.9, 0.9, 0.9)),
             s.MakeBox((0.2, -1.0, 1.6), (1.0, -0.2, 2.4), mats[3])]
    _room(s, [s.BvhNode(balls), s.BvhNode(comps)], world="list")


@nesting
def instance_of_a_bvh_of_composites(s, Rng):
    """RotateY(BvhNode[boxes, instanced boxes, a medium]): the sub-tree is walked in the reference's order inside the
    instance, media leaves (incl. a span-1 one) drawing as they are met."""
    white, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.12, 0.45, 0.15))
    members = [s.MakeBox((-2.4, -1, -0.4), (-1.6, 0.3, 0.4), white),
               s.Translate(s.MakeBox((0, 0, 0), (0.7, 0.7, 0.7), green), (-0.9, -1.0, 0.3)),
               s.ConstantMedium(s.MakeBox((0.3, -1.0, -0.5), (1.3, 0.5, 0.5), white), 2.0, (0.8, 0.8, 0.8)),
               s.Sphere((2.1, -0.4, 0.0), 0.6, s.Dielectric(1.5)),
               s.ConstantMedium(s.Sphere((3.4, -0.3, 0.2), 0.7, white), 1.2, (0.9, 0.4, 0.1))]
    tree = s.BvhNode(members)
    _room(s, [s.Translate(s.RotateY(tree, -12.0), (-0.4, 0.0, -0.6))])


@nesting
def many_chained_transforms(s, Rng):
    """Eleven chained Translate / RotateY wrappers around one box (the reference recurses without a limit)."""
    obj = s.MakeBox((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6), s.Lambertian((0.8, 0.5, 0.2)))
    for k in range(11):
        obj = s.RotateY(obj, 7.0 + k) if k % 2 == 0 else s.Translate(obj, (0.11 * k, 0.02 * k, -0.05 * k))
    _room(s, [obj, s.Sphere((-2.2, 0, 0), 1.0, s.Lambertian(s.NoiseTexture(3.0, Rng(1984, 0))))])


@nesting
def list_of_lists_world(s, Rng):
    """A HittableList world holding HittableLists of mixed members, three levels deep, plus a lone medium."""
    white = s.Lambertian((0.73, 0.73, 0.73))
    inner = s.HittableList([s.Sphere((-1.5, -0.4, 0), 0.6, s.Metal((0.9, 0.6, 0.3), 0.3)),
                            s.HittableList([s.Quad((-0.5, -1, -1), (1, 0, 0), (0, 1.6, 0), white),
                                            s.ConstantMedium(s.Sphere((1.5, -0.2, 0.5), 0.8, white), 1.8, (0.4, 0.7, 0.9))])])
    _room(s, [s.HittableList([inner, s.MakeBox((2.6, -1, -1), (3.4, 0.4, -0.2), white)])], world="list")


@nesting
def bvh_object_among_the_leaves_of_a_bvh_world(s, Rng):
    """BvhNode world whose leaves include a BvhNode OBJECT over composites: the reference's loop walks it as part of the
    world's own tree (IsBvhNode), leaf siblings first -- not as a leaf call.  (_room builds the BvhNode world.)"""
    white = s.Lambertian((0.73, 0.73, 0.73))
    inner = s.BvhNode([s.ConstantMedium(s.Sphere((-1.6, 0.0, 0.3), 0.8, white), 1.6, (0.8, 0.3, 0.2)),
                       s.MakeBox((-0.4, -1.0, -0.5), (0.5, 0.4, 0.4), white),
                       s.ConstantMedium(s.MakeBox((0.9, -1.0, -0.6), (1.9, 0.7, 0.5), white), 1.1, (0.2, 0.3, 0.8))])
    _room(s, [inner, s.Sphere((3.0, 0.0, -0.5), 0.9, s.Metal((0.8, 0.8, 0.8), 0.05)),
              s.ConstantMedium(s.Sphere((-3.2, 0.2, -0.8), 0.9, white), 0.9, (0.9, 0.9, 0.9))])


@pytest.mark.parametrize("name", sorted(NESTINGS))
def test_general_nesting_matches_the_oracle(name):
    check(NESTINGS[name], spp=6, min_exact=0.97)


# ---- sphere-list filter under cancellation ----
def _far_sphere_list(offset, n=40, touching=True):
    def build(s, Rng):
        ox, oy, oz = offset
        rnd = np.random.default_rng(5)
        items = []
        # a wall of touching spheres (silhouettes everywhere: rays that graze), some glass, a huge ground sphere
        for k in range(n):
            cx, cy = (k % 8) * 0.5 - 1.75, (k // 8) * 0.5 - 1.0
            r = 0.25 if touching else 0.2
            mat = s.Dielectric(1.5) if k % 5 == 0 else (s.Metal(tuple(rnd.uniform(0.4, 0.9, 3)), 0.0) if k % 3 == 0
                                                         else s.Lambertian(tuple(rnd.uniform(0.1, 0.9, 3))))
            items.append(s.Sphere((ox + cx, oy + cy, oz - 4.0), r, mat))
        items.append(s.Sphere((ox, oy - 1000.5 - 1.0, oz - 4.0), 1000.0, s.Lambertian((0.5, 0.5, 0.5))))
        s.SetWorld(s.HittableList(items))
        s.Camera((ox, oy, oz), (ox, oy, oz - 4.0), (0, 1, 0), 50, 96 / 64, 0.0, 10.0)
        s.Commit()
    return build


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (3000.0, -2000.0, 5000.0), (1.0e6, 2.0e6, -3.0e6)])
def test_sphere_list_filter_far_from_the_origin(offset):
    """The list scan's conservative filter expands (o - C)^2 around the world origin, so a scene far away from it is where
    cancellation would bite: its margin grows with (|o| + |C| + r)^2 and the filter passes more spheres, never fewer.
    Strict build = oracle bit for bit (the oracle runs the reference's discriminant on every sphere), ray counts equal, and
    the exact scan (RT_FLAG_EXACT_SCAN) gives the same frame in both builds."""
    import raytracinginoneweekendincuda_amd as rt
    w, h, spp = 96, 64, 8
    prod, orc = build_both(_far_sphere_list(offset))
    want, stats = orc.render(w, h, spp, want_stats=True)
    for variant in (0, 1):
        got, st = prod.render(w, h, spp, variant=variant)
        ref, st_ref = prod.render(w, h, spp, variant=variant, flags=rt.FLAG_EXACT_SCAN)
        assert st.kernel_kind == 16
        assert st.rays == st_ref.rays and np.array_equal(got.view(np.uint64), ref.view(np.uint64))
        if variant == 0:
            assert st.rays == stats["rays"]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---- scenes too big for the LDS-only kernels fall back to the kernels that read from L2 ----
def test_library_tree_kernel_falls_back_when_its_rows_do_not_fit():
    """The library-tree kernel (768-thread workgroup) reads sphere, moving-sphere and material rows from LDS only and is
    launched only when all of them fit beside the node rows; 600 moving spheres with a material each need 173 KB, so the
    reference-tree kernel renders this world -- same frame as the oracle's."""
    def build(s, Rng):
        rnd = np.random.default_rng(11)
        items = []
        for k in range(600):
            c = rnd.uniform(-6, 6, 3)
            c[2] -= 12.0
            mat = s.Lambertian(tuple(rnd.uniform(0.1, 0.9, 3))) if k % 3 else s.Metal(tuple(rnd.uniform(0.4, 0.9, 3)), 0.1)
            items.append(s.MovingSphere(tuple(c), tuple(c + np.array([0.0, 0.2, 0.0])), 0.0, 1.0, 0.25, mat))
        s.SetWorld(s.BvhNode(items))
        s.Camera((0, 0, 2), (0, 0, -12), (0, 1, 0), 50, W / H, 0.0, 10.0, 0.0, 1.0)
        s.Commit()
    prod, orc = build_both(build)
    want, stats = orc.render(W, H, SPP, want_stats=True)
    got, st = prod.render(W, H, SPP, variant=0)
    assert (st.kernel_kind & 64) == 0, "the library-tree kernel cannot hold this world's rows"
    assert st.rays == stats["rays"]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_deep_kernel_falls_back_when_its_tables_do_not_fit():
    """The kind-batched deep kernel reads its node rows and tables from LDS only; 700 boxes (106 KB of box rows) exceed its
    budget, so the general kernel (two waves per SIMD, rows from L2) renders the scene."""
    def build(s, Rng):
        rnd = np.random.default_rng(12)
        ground = s.Lambertian((0.48, 0.83, 0.53))
        items = []
        for k in range(700):
            x, z = (k % 28) * 1.0 - 14.0, (k // 28) * 1.0 - 30.0
            items.append(s.MakeBox((x, -2.0, z), (x + 0.9, -2.0 + float(rnd.uniform(0.1, 1.0)), z + 0.9), ground))
        items.append(s.Sphere((0, 1, -12), 1.5, s.Lambertian(s.NoiseTexture(0.2, Rng(1984, 5)))))
        items.append(s.Sphere((0, 8, -10), 2.0, s.DiffuseLight((7, 7, 7))))
        s.SetWorld(s.BvhNode(items))
        s.Camera((0, 2, 4), (0, 0, -12), (0, 1, 0), 50, W / H, 0.0, 10.0, 0.0, 1.0, (0.1, 0.1, 0.1))
        s.Commit()
    prod, orc = build_both(build)
    want, stats = orc.render(W, H, SPP, want_stats=True)
    got, st = prod.render(W, H, SPP, variant=0)
    print(f"kernel kind {st.kernel_kind}, vgprs {st.kernel_vgprs}")
    assert st.kernel_vgprs > 168, "the 768-thread deep kernel (168 VGPRs) cannot hold 700 box rows"
    assert st.rays == stats["rays"]
    exact, within, worst = compare(got, want, TOL)
    assert within >= 0.999 and exact >= 0.95   # Perlin: device sin differs from glibc's by an ulp in a few pixels
