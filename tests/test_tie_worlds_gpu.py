"""Ties between box faces, instances and resting spheres on the GPU: every walk and scan that meets the leaves in an order
of its own must still show what the reference's order shows.

The worlds are those of tests/tie_worlds.py (tests/test_tie_worlds_host.py shows with the oracle alone that the order of each
tied pair decides at least 0.5 % of their pixels).  The sharp assertion throughout is bit-equality between a render that may use
one of the library's own search structures and one that walks the reference's tree / scans the reference's list in its order: a
single mis-decided tie fails it.  The strict build is held against the oracle as well, in the acceptance shape of
test_custom_scenes_gpu.test_segmented_walk_matches_the_oracle_and_the_reference_order_walk, and the ray queries against
closed forms: t from the geometry, the winning leaf from the reference's rule (the later of two tied quads or boxes, the
earlier of two tied spheres)."""
import numpy as np
import pytest

import tie_worlds as T
from conftest import build_both
from frame_helpers import compare

pytestmark = pytest.mark.gpu

SIDES = sorted(T.SIDES)
SPHERE_PAIRS = [p for p in T.PAIRS if T.PAIRS[p][1] == "sphere"]


def against_the_oracle(what, got, st, want, stats):
    exact, within, _ = compare(got, want)
    print(f"{what}: kernel kind {st.kernel_kind}, bit-exact {exact:.4f}, within {within:.4f}")
    assert st.rays == stats["rays"], (what, st.rays, stats["rays"])
    assert within >= 0.999 and exact >= 0.98, (what, exact, within)


def same_frames(what, renders):
    """renders: [(label, frame, stats)]; all bit-equal to the first, with its ray count."""
    label0, frame0, st0 = renders[0]
    for label, frame, st in renders[1:]:
        differ = T.differing(frame, frame0)
        assert st.rays == st0.rays and differ == 0.0, \
            f"{what}: {label} (kernel kind {st.kernel_kind}) differs from {label0} (kernel kind {st0.kernel_kind}) in {differ:.4f} of the pixels"


# ---- deep worlds: the segmented walk / the library's tree against the reference's tree ----
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pair", T.COMPOSITE)
def test_deep_composite_world(pair, side, swap):
    prod, orc = build_both(T.tie_world(pair, "bvh", swap, side=side))
    want, stats = orc.render(T.W, T.H, T.SPP, want_stats=True)
    for variant in (0, 1):
        seg, st = prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_FORCE_GENERAL)
        ref, st_ref = prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_FORCE_GENERAL | T.FLAG_REFERENCE_TREE)
        assert st_ref.kernel_kind == 7
        same_frames(f"{pair} {side} swap={swap} build {variant}", [("the reference's tree", ref, st_ref), ("flags=2", seg, st)])
        if variant == 0:
            against_the_oracle(f"{pair} {side} swap={swap}", seg, st, want, stats)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pair", ["floor_under_glass", "tops", "instanced"])
def test_deep_composite_world_with_fog_beside_the_pair(pair, side):
    """A ConstantMedium whose padded box reaches the pair: the candidate lists of the segmented walk (render.hip seg_advance)."""
    prod, orc = build_both(T.tie_world(pair, "bvh", side=side, media=True))
    want, stats = orc.render(T.W, T.H, 6, want_stats=True)
    for variant in (0, 1):
        seg, st = prod.render(T.W, T.H, 6, variant=variant, flags=T.FLAG_FORCE_GENERAL)
        ref, st_ref = prod.render(T.W, T.H, 6, variant=variant, flags=T.FLAG_FORCE_GENERAL | T.FLAG_REFERENCE_TREE)
        same_frames(f"{pair} + fog {side} build {variant}", [("the reference's tree", ref, st_ref), ("flags=2", seg, st)])
        if variant == 0:
            against_the_oracle(f"{pair} + fog {side}", seg, st, want, stats)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pair", SPHERE_PAIRS)
def test_sphere_pair_in_a_bvh_world(pair, side, swap):
    prod, orc = build_both(T.tie_world(pair, "bvh", swap, side=side))
    want, stats = orc.render(T.W, T.H, T.SPP, want_stats=True)
    for variant in (0, 1):
        got, st = prod.render(T.W, T.H, T.SPP, variant=variant)
        ref, st_ref = prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_REFERENCE_TREE)
        assert st_ref.kernel_kind == 0
        same_frames(f"{pair} {side} swap={swap} build {variant}", [("the reference's tree", ref, st_ref), ("default", got, st)])
        if variant == 0:
            against_the_oracle(f"{pair} {side} swap={swap}", got, st, want, stats)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pair", SPHERE_PAIRS)
def test_sphere_pair_in_a_list_world(pair, side, swap):
    prod, orc = build_both(T.tie_world(pair, "list", swap, side=side))
    want, stats = orc.render(T.W, T.H, T.SPP, want_stats=True)
    for variant in (0, 1):
        plain, st = prod.render(T.W, T.H, T.SPP, variant=variant)
        assert st.kernel_kind == 8
        renders = [("the list scan", plain, st)]
        renders.append(("RT_FLAG_ACCELERATE_LISTS",) + prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_ACCELERATE_LISTS))
        for ppw in (16, 4, 1):
            renders.append((f"pixels_per_wave {ppw}",) + prod.render(T.W, T.H, T.SPP, variant=variant, pixels_per_wave=ppw))
            assert renders[-1][2].kernel_kind & 128
        same_frames(f"{pair} list {side} swap={swap} build {variant}", renders)
        if variant == 0:
            against_the_oracle(f"{pair} list {side} swap={swap}", plain, st, want, stats)


# ---- small worlds: the scan in leaf order, the walk, the lanes-per-ray reduction ----
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("pair", sorted(T.PAIRS))
def test_small_world(pair, side, swap):
    """At most 16 leaves: a BvhNode world is scanned in leaf order (kinds 10 / 8) or, with RT_FLAG_ALWAYS_WALK, walked; a list
    world is scanned, one lane per ray or several (the reduction's tie key was written for quads and spheres: box faces and
    instances must obey it too).  All renders of a world are bit-equal, the strict one is the oracle's frame of that world, and
    the two worlds give one frame where the oracle's two do."""
    composite = T.PAIRS[pair][1] == "plane"
    scans, wants = {}, {}
    for world in ("bvh", "list"):
        prod, orc = build_both(T.tie_world(pair, world, swap, fillers=6, side=side))
        want, stats = orc.render(T.W, T.H, T.SPP, want_stats=True)
        wants[world] = want
        for variant in (0, 1):
            plain, st = prod.render(T.W, T.H, T.SPP, variant=variant)
            assert st.kernel_kind == (10 if composite else 8)
            renders = [("the scan", plain, st)]
            if world == "bvh":
                renders.append(("RT_FLAG_ALWAYS_WALK",) + prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_ALWAYS_WALK))
                renders.append(("walk of the reference's tree",) + prod.render(T.W, T.H, T.SPP, variant=variant,
                                                                               flags=T.FLAG_ALWAYS_WALK | T.FLAG_REFERENCE_TREE))
                assert renders[-1][2].kernel_kind == (2 if composite else 0)
            else:
                for ppw in (16, 4, 1):
                    renders.append((f"pixels_per_wave {ppw}",) + prod.render(T.W, T.H, T.SPP, variant=variant, pixels_per_wave=ppw))
                    assert renders[-1][2].kernel_kind & 128
            same_frames(f"small {pair} {world} {side} swap={swap} build {variant}", renders)
            if variant == 0:
                against_the_oracle(f"small {pair} {world} {side} swap={swap}", plain, st, want, stats)
            scans[world, variant] = plain
    # the reference's BvhNode sorts its leaves, so its frame need not be its list's; where the oracle says it is, it is here too
    if T.differing(wants["bvh"], wants["list"]) == 0.0:
        for variant in (0, 1):
            assert T.differing(scans["bvh", variant], scans["list", variant]) == 0.0, (pair, side, swap, variant)


# ---- a twin inside a group: the sub-BVH and the cooperative scan ----
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("twin", ["static", "resting", "resting_apart"])
def test_twin_inside_a_group(twin, side, swap):
    for world in ("bvh", "list"):
        prod, orc = build_both(T.group_world(twin, world, swap, side=side))
        want, stats = orc.render(T.W, T.H, T.SPP, want_stats=True)
        for variant in (0, 1):
            got, st = prod.render(T.W, T.H, T.SPP, variant=variant)
            renders = [("default", got, st)]
            renders.append(("flags=2|128",) + prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_FORCE_GENERAL | T.FLAG_REFERENCE_TREE))
            if world == "bvh":
                renders.append(("flags=2",) + prod.render(T.W, T.H, T.SPP, variant=variant, flags=T.FLAG_FORCE_GENERAL))
            same_frames(f"group {twin} {world} {side} swap={swap} build {variant}", renders)
            if variant == 0:
                against_the_oracle(f"group {twin} {world} {side} swap={swap}", got, st, want, stats)


# ---- a reference that is not the oracle: closed forms through the ray queries ----
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("pair", sorted(T.PAIRS))
def test_ray_queries_return_the_leaf_the_references_rule_names(pair, swap):
    """Rays straight onto the overlap of the pair in the LIST worlds (leaves 0 and 1 are the pair): t is known in closed form, and
    the winning leaf is the later of two tied quads or boxes, the earlier of two tied spheres -- and the static sphere where the
    moving one's clock stands still.  Batches of 1 and 65 rays; occluded() agrees."""
    import raytracinginoneweekendincuda_amd as rt
    ties, what = T.PAIRS[pair]
    if not ties:
        leaf = 1 if swap else 0      # the Sphere, wherever it stands
    else:
        leaf = 1 if what == "plane" else 0
    origin, direction, t = T.PROBES[pair]
    s = rt.Scene()
    T.tie_world(pair, "list", swap)(s, rt.Rng)
    for variant in (0, 1):
        for count in (1, 65):
            o = np.tile(np.array(origin, dtype=np.float64), (count, 1))
            if what == "plane":
                o[:, 0] += np.arange(count) / 256.0   # along x inside the overlap: the planes are flat, t stays
            d = np.tile(np.array(direction, dtype=np.float64), (count, 1))
            out = s.intersect(o, d, time=0.5, variant=variant, want=("t", "leaf"))
            assert np.array_equal(out["t"], np.full(count, t)), (pair, swap, variant, out["t"][:4])
            assert (out["leaf"] == leaf).all(), (pair, swap, variant, count, out["leaf"][:8])
            assert s.occluded(o, d, time=0.5, variant=variant).all()
            assert not s.occluded(o, d, time=0.5, variant=variant, tmax=t * 0.5).any()
