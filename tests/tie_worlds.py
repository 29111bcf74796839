"""Worlds in which two surfaces answer a ray with the same t bit for bit, so that the ORDER of the tests decides what the ray
sees: a later quad or box face wins (R/Quad.h:64 rejects only t > tMax, R/HittableList.h:44-51 hands closestSoFar on), a later
sphere does not (R/Sphere.h:38,50 is strict).  The library's own accelerators meet leaves in another order than the reference
does, and csrc/scene_builder.cpp has_coincident_primitives keeps them off such worlds.  The builders here place the ties that
guard has to see -- box faces, instances, a moving sphere that rests -- and the controls it must leave alone; they are shared
by tests/test_tie_worlds_host.py (oracle and launch plan, no GPU) and tests/test_tie_worlds_gpu.py.  Not a test module.

Every coordinate of a tied surface, of a Translate offset and of a camera origin is dyadic, so primary rays tie exactly;
whether a secondary ray ties is the reference's arithmetic's business, and the oracle decides it."""
import numpy as np

W, H, SPP = 64, 48, 4

FLAG_FORCE_GENERAL, FLAG_ALWAYS_WALK, FLAG_REFERENCE_TREE, FLAG_ACCELERATE_LISTS = 2, 32, 128, 512

# the camera on each side of the scene, eight units from the point (0.5, 0, 0) it looks at and six above it: the library's
# trees are threaded by ray octant, so what the reference's fixed left-then-right order agrees with on one side it does not on
# the opposite one
SIDES = {"+z": (0.5, 6.0, 8.0), "-z": (0.5, 6.0, -8.0), "+x": (8.5, 6.0, 0.0), "-x": (-7.5, 6.0, 0.0)}
LOOK_AT = (0.5, 0.0, 0.0)
LIFT = [0.0]   # tie_world(untied=True) builds with 2^-10 here: the second of a composite pair is raised by it, nothing ties

# pair name -> (does the pair tie at all, kind of the tied surfaces: "plane" = the later one wins, "sphere" = the earlier)
PAIRS = {
    "floor_under_glass": (True, "plane"),    # a glass block standing on a floor quad: its bottom face lies in the floor
    "tops": (True, "plane"),                 # two boxes of one height that overlap: equal tops
    "instanced": (True, "plane"),            # a mirror quad on top of a translated box
    "spheres": (True, "sphere"),             # a sphere and a moving sphere that rests in the same place
    "twin_boxes": (True, "plane"),           # the same box twice, two materials
    "box_and_moved_box": (True, "plane"),    # top and front face of a box in the planes of those of a translated one
    "rotated": (True, "plane"),              # a quad on top of a box rotated by 90 degrees, then translated (y is untouched)
    "stopped_clock": (False, "sphere"),      # a moving sphere with time0 == time1: frac is inf / NaN, it is never hit
}
COMPOSITE = [p for p in PAIRS if PAIRS[p][1] == "plane"]
# the pairs of the issue's table (order dependence measured there) and the further ones
MAIN = ["floor_under_glass", "tops", "instanced", "spheres"]

# rays straight down onto (or, for the spheres, straight at) the overlap of every pair: origin, direction, t in closed form
PROBES = {
    "floor_under_glass": ((0.25, -4.0, 0.5), (0.0, 1.0, 0.0), 4.0),    # from below: the floor and the block's bottom at y = 0
    "tops": ((3.5, 5.0, 0.25), (0.0, -1.0, 0.0), 4.0),
    "instanced": ((-4.0, 5.0, 2.5), (0.0, -1.0, 0.0), 4.0),
    "spheres": ((0.0, 5.0, 0.0), (0.0, -1.0, 0.0), 3.0),
    "twin_boxes": ((0.25, 5.0, 0.5), (0.0, -1.0, 0.0), 3.5),
    "box_and_moved_box": ((1.5, 5.0, 0.0), (0.0, -1.0, 0.0), 4.0),     # (the front faces in z = 1 and the bottoms tie as well)
    "rotated": ((-4.0, 5.0, 2.5), (0.0, -1.0, 0.0), 4.0),
    "stopped_clock": ((0.0, 5.0, 0.0), (0.0, -1.0, 0.0), 3.0),
}


def _pair(s, name):
    """(the two tied hittables in list order A, the centre of a ball of fog that reaches them, companions).  A surface-area
    tree puts two leaves whose boxes overlap into one bottom node when everything else is small and far away, and there they are
    tested in list order whatever the ray's octant.  The companions are leaves that stand closer to one of the pair than the
    other one of the pair does, so that the library's tree separates the two (tests/test_tie_worlds_host.py checks that it
    does, on the same world with one of the pair moved by 2^-10): only then does the visiting order depend on the octant.
    Two identical boxes, or identical spheres, cannot be separated this way."""
    red, green, grey = s.Lambertian((0.8, 0.1, 0.1)), s.Lambertian((0.1, 0.8, 0.1)), s.Lambertian((0.5, 0.5, 0.6))
    if name == "floor_under_glass":
        floor = s.Quad((-8.0, 0.0, -8.0), (16.0, 0.0, 0.0), (0.0, 0.0, 16.0), s.Lambertian((0.8, 0.8, 0.8)))
        block = s.MakeBox((-1.0, 0.0 + LIFT[0], -1.0), (1.0, 2.0, 1.0), s.Dielectric(1.5))
        return [floor, block], (0.0, 2.5, 0.0), [s.MakeBox((1.5, 0.25, -0.5), (2.5, 1.25, 0.5), grey)]
    if name == "tops":
        pair = [s.MakeBox((2.0, 0.0, -1.0), (4.0, 1.0, 1.0), red), s.MakeBox((3.0, 0.0 + LIFT[0], -0.5), (5.0, 1.0 + LIFT[0], 0.5), green)]
        return pair, (3.5, 1.75, 0.0), [s.MakeBox((1.25, 0.25, -0.5), (1.75, 0.75, 0.5), grey), s.MakeBox((5.25, 0.25, -0.25), (5.75, 0.75, 0.25), grey)]
    if name in ("instanced", "rotated"):
        # a mirror platform on a pedestal: the pedestal's top lies in the platform.  "rotated": RotateY by 90 degrees maps (x, z)
        # to (z, -x) up to the rounding of cos(pi / 2), the same pedestal after the move; y is untouched
        if name == "instanced":
            box = s.Translate(s.MakeBox((0.0, 0.0, 0.0), (2.0, 1.0, 2.0), red), (-5.0, 0.0, 1.5))
        else:
            box = s.Translate(s.RotateY(s.MakeBox((0.0, 0.0, 0.0), (2.0, 1.0, 2.0), red), 90.0), (-5.0, 0.0, 3.5))
        platform = s.Quad((-6.0, 1.0 + LIFT[0], 0.5), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), s.Metal((0.9, 0.9, 0.9), 0.0))
        return [box, platform], (-4.0, 1.75, 2.5), [s.MakeBox((-2.75, 0.0, 2.0), (-2.25, 0.75, 3.0), grey)]
    if name == "spheres":
        return [s.Sphere((0.0, 1.0, 0.0), 1.0, red), s.MovingSphere((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.0, 1.0, 1.0, green)], (0.0, 2.5, 0.0), []
    if name == "twin_boxes":
        return [s.MakeBox((-1.0, 0.0, -1.0), (1.0, 1.5, 1.0), red), s.MakeBox((-1.0, 0.0, -1.0), (1.0, 1.5, 1.0), green)], (0.0, 2.25, 0.0), []
    if name == "box_and_moved_box":
        moved = s.Translate(s.MakeBox((0.0, 0.0, 0.0), (2.0, 1.0, 2.0), green), (1.0, 0.0 + LIFT[0], -1.0 + LIFT[0]))   # (top, bottom, front and back all tie)
        return [s.MakeBox((-1.0, 0.0, -1.0), (2.0, 1.0, 1.0), red), moved], (1.5, 1.75, 0.0), \
               [s.MakeBox((-1.75, 0.25, -0.5), (-1.25, 0.75, 0.5), grey), s.MakeBox((3.25, 0.25, -0.5), (3.75, 0.75, 0.5), grey)]
    if name == "stopped_clock":
        return [s.Sphere((0.0, 1.0, 0.0), 1.0, red), s.MovingSphere((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.5, 0.5, 1.0, green)], (0.0, 2.5, 0.0), []
    raise KeyError(name)


def _fillers(s, n):
    """n small spheres in rows around the scene, none of them near a pair: they only make the world deep."""
    mats = [s.Lambertian((0.7, 0.3, 0.2)), s.Lambertian((0.2, 0.4, 0.8)), s.Metal((0.8, 0.8, 0.7), 0.1), s.Lambertian((0.3, 0.7, 0.3))]
    spots = [(x + 0.5, z) for z in (-5.0, 5.0, -6.0, 6.0, -7.0, 7.0) for x in range(-8, 8)]
    assert n <= len(spots)
    return [s.Sphere((x, 0.25, z), 0.25, mats[k % 4]) for k, (x, z) in enumerate(spots[:n])]


def _finish(s, items, world, side):
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera(SIDES[side], LOOK_AT, (0, 1, 0), 45.0, W / H, 0.0, 10.0, 0.0, 1.0)
    s.Commit()


def tie_world(pair, world="bvh", swap=False, fillers=72, side="+z", media=False, untied=False):
    """One pair and `fillers` small spheres: 72 make a BvhNode world deeper than csrc/launch_plan.cpp kDeepWorldNodes, 6 one of at
    most 16 leaves.  `swap`: the pair's list order reversed.  `media`: a ball of thin fog whose box reaches the pair (cameras
    outside it, scattered rays inside it) -- the candidate lists of the segmented walk.  `untied`: the control, one of a
    composite pair moved by 2^-10 so that nothing ties.  The pair comes first in the list: a list world's leaves 0 and 1."""
    def build(s, Rng):
        LIFT[0] = 0.0009765625 if untied else 0.0
        try:
            items, fog_at, companions = _pair(s, pair)
        finally:
            LIFT[0] = 0.0
        build.pair = tuple(items)   # handles, for separated_by_the_library_tree
        if swap:
            items.reverse()
        if media:
            items.append(s.ConstantMedium(s.Sphere(fog_at, 1.0, s.Dielectric(1.5)), 0.4, (0.9, 0.9, 0.9)))
        _finish(s, items + companions + _fillers(s, fillers), world, side)
    return build


def group_world(twin, world="bvh", swap=False, side="+z", fillers=6):
    """Translate(HittableList(20 spheres)): the group that gets a sub-BVH of its own (flat_scene.h kSubBvhMinPrims) and, all of
    them static, the cooperative scan.  Two of the twenty lie in one place: `twin` = "static" (the same Sphere twice),
    "resting" (a Sphere and a MovingSphere that does not move); the controls "none" and "resting_apart": the second one, a Sphere
    or a resting MovingSphere, stands apart."""
    def build(s, Rng):
        rnd = np.random.default_rng(31)
        red, green = s.Lambertian((0.8, 0.1, 0.1)), s.Lambertian((0.1, 0.8, 0.1))
        mats = [s.Lambertian((0.7, 0.6, 0.2)), s.Metal((0.8, 0.8, 0.9), 0.0), s.Lambertian((0.2, 0.3, 0.8))]
        c = (0.5, 1.0, 0.0)
        first = s.Sphere(c, 1.0, red)
        if twin == "resting":
            second = s.MovingSphere(c, c, 0.0, 1.0, 1.0, green)
        elif twin == "resting_apart":
            second = s.MovingSphere((0.5, 1.0, -2.5), (0.5, 1.0, -2.5), 0.0, 1.0, 1.0, green)
        else:
            second = s.Sphere(c if twin == "static" else (0.5, 1.0, -2.5), 1.0, green)
        pair = [second, first] if swap else [first, second]
        members = []
        for k in range(18):
            members.append(s.Sphere((-3.0 + 0.5 * (k % 9) + (5.0 if k % 9 > 3 else 0.0), 0.25 + 0.5 * (k // 9), float(rnd.integers(-8, 9)) / 4.0),
                                    0.25, mats[k % 3]))
        members[9:9] = pair   # in the middle of the list
        group = s.Translate(s.HittableList(members), (0.5, 0.25, -0.5))
        floor = s.Quad((-8.0, 0.0, -8.0), (16.0, 0.0, 0.0), (0.0, 0.0, 16.0), s.Lambertian((0.8, 0.8, 0.8)))
        _finish(s, [group, floor] + _fillers(s, fillers), world, side)
    return build


# ---- controls: worlds without a reachable tie, which keep their accelerators ----
def abutting_boxes(world="bvh", side="+z", scale=1.0):
    """A field of opaque boxes as the ground of the Book-2 final scene: one box's +x face is the next one's -x face (and +z / -z
    likewise), their bottoms lie in one plane and touch along edges, their tops differ.  No ray from outside the solids reaches
    the shared part of two faces; plus a few spheres and one instanced box so that the world is a deep composite one."""
    def build(s, Rng):
        rnd = np.random.default_rng(9)
        ground = s.Lambertian((0.48, 0.83, 0.53))
        items = []
        at = [(-8.0 + 2.0 * i) * scale for i in range(9)]   # (a scale like 0.7: extents that round, neighbours still share their bits)
        for i in range(8):
            for k in range(8):
                items.append(s.MakeBox((at[i], -2.0, at[k]), (at[i + 1], -2.0 + float(rnd.integers(1, 9)) / 8.0, at[k + 1]), ground))
        items.append(s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.0, 1.5, 1.0), s.Lambertian((0.7, 0.7, 0.7))), 20.0), (-2.0, 0.5, 1.0)))
        items += _fillers(s, 8)
        _finish(s, items, world, side)
    return build


def separate_tops(world="bvh", side="+z"):
    """Boxes of one height that stand apart, and two that touch along an edge: coplanar tops (and bottoms) that do not overlap."""
    def build(s, Rng):
        red, green = s.Lambertian((0.8, 0.1, 0.1)), s.Lambertian((0.1, 0.8, 0.1))
        items = [s.MakeBox((2.0, 0.0, -1.0), (3.0, 1.0, 1.0), red), s.MakeBox((3.5, 0.0, -0.5), (5.0, 1.0, 0.5), green),
                 s.MakeBox((-3.0, 0.0, 0.0), (-2.0, 1.0, 1.0), red), s.MakeBox((-2.0, 0.0, 1.0), (-1.0, 1.0, 2.0), green),
                 s.Translate(s.MakeBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), red), (-4.0, 0.0, -3.0))]
        _finish(s, items + _fillers(s, 72), world, side)
    return build


def lone_resting_sphere(world="bvh", side="+z", fillers=18):
    """A moving sphere that rests, with nothing in its place: nothing ties."""
    def build(s, Rng):
        items = [s.MovingSphere((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 0.0, 1.0, 1.0, s.Lambertian((0.1, 0.8, 0.1)))]
        _finish(s, items + _fillers(s, fillers), world, side)
    return build


def separated_by_the_library_tree(scene, build):
    """Does the library's tree of a committed product scene hold the two of `build`'s pair in different bottom nodes?  A bottom
    node's box is the union of its two leaves' boxes, so the pair shares one exactly where a bottom node has the union of theirs."""
    boxes, ab, _ = scene.dump_fast_nodes()
    assert boxes.shape[0] > 0, "no library tree"
    a, b = (np.array(scene.BoundingBox(h)) for h in build.pair)
    union = np.where(np.arange(6) % 2 == 0, np.minimum(a, b), np.maximum(a, b))   # {xmin, xmax, ymin, ymax, zmin, zmax}
    bottom = (ab[:, 0] >> 28) != 14
    return not any(np.array_equal(box, union) for box in boxes[bottom])


# ---- comparisons ----
def differing(a, b):
    """Share of the pixels in which two frames differ in any bit."""
    return float(np.mean(np.any(a.view(np.uint64) != b.view(np.uint64), axis=-1)))
