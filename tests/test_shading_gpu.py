"""What happens after the hit -- make_surface, texture_value, material_texture, perlin_noise / perlin_noise_lds and shade
(csrc/render.hip), lower_materials (csrc/scene_builder.cpp) -- for every texture and material kind through every shading
kernel.  The scenes are written once and built on both sides (conftest.build_both); the reference of every comparison is
the CPU oracle (fp64 restatement of the reference's arithmetic) or the library's own invariant that kernel choice and
scheduling never change a bit.  Which kernel ran is asserted from RenderStats.kernel_kind
(world*8 + media*4 + composite*2 + rich + nested*32 + library-tree*64 + grouped*128 + segmented*256).

  part 1  texture x carrier against the oracle          test_texture_on_every_carrier_*, test_textured_carriers_bvh_world_*
  part 2  the rich kernels against each other           test_deep_rich_*, test_nested_kernels_*
  part 3  the non-rich kernels with inline textures     test_inline_textures_*
  part 4  material parameters at their edges            test_material_edges_*

tests/test_shading_host.py holds the checks that need no GPU (the scenes commit, table counts, boxes, leaf order, and that
every edge material of part 4 is really in view).
"""
import numpy as np
import pytest

from conftest import build_both
from frame_helpers import compare
from query_helpers import bits

pytestmark = pytest.mark.gpu

W, H = 96, 64

FLAG_KEEP_RNG_STATE, FLAG_FORCE_GENERAL, FLAG_ACCUMULATE, FLAG_ALWAYS_WALK = 1, 2, 8, 32
FLAG_NO_PIXEL_CLASSES, FLAG_REFERENCE_TREE, FLAG_EXACT_SCAN, FLAG_FILTER_FP64 = 64, 128, 256, 2048


# ------------------------------------------------------------------------------------------------------------------
# textures
# ------------------------------------------------------------------------------------------------------------------
# Random bytes from a fixed seed: a one-texel slip changes the colour by a lot.  Creation order = IMAGE_ORDER, the largest
# not first, so ImageRec.offset is non-zero for every image but the 2 x 3 one.
IMAGE_SIZES = {"img2x3": (2, 3), "img256x128": (256, 128), "img1x1": (1, 1), "img37x19": (37, 19)}
IMAGE_ORDER = ("img2x3", "img256x128", "img1x1", "img37x19")
IMAGE_BYTES = sum(w * h * 3 for w, h in IMAGE_SIZES.values())


def images():
    rng = np.random.default_rng(3)
    return {name: rng.integers(0, 256, (IMAGE_SIZES[name][1], IMAGE_SIZES[name][0], 3), dtype=np.uint8) for name in IMAGE_ORDER}


TEXTURES = ("img1x1", "img2x3", "img37x19", "img256x128", "cyan", "noise", "chk_solid", "chk_chk", "chk_img_noise")
READS_UV = ("img1x1", "img2x3", "img37x19", "img256x128", "cyan", "chk_img_noise")   # an ImageTexture somewhere in the tree
PLAIN = ("chk_solid",)   # lower_materials resolves it into the material row: SCENE_RICH_TEXTURES stays clear


def make_texture(s, Rng, name):
    """-> (texture under test, the texture for the phase functions of the scene's media).

    ConstantMedium::Hit never writes U / V (R/ConstantMedium.h:86-91), so a phase texture that reads them sees whatever the
    record held before: undefined in the reference, stale in the oracle, 0 in make_surface.  Media therefore carry only
    textures that ignore u, v: the noise, the checkers of solids, and -- in the checker(image, noise) scene -- a checker of
    the noise and a solid.  The scenes of the image textures have no media."""
    sol = lambda *c: s.SolidColor(c)
    if name == "chk_solid":      # no image and no noise may even exist in this scene: every one of them makes it rich
        t = s.CheckerTexture(0.5, sol(0.9, 0.1, 0.1), sol(0.1, 0.1, 0.9))
        return t, t
    if name == "chk_chk":        # texture_value's table walk, two levels
        t = s.CheckerTexture(2.0, s.CheckerTexture(0.5, sol(0.9, 0.1, 0.1), sol(0.1, 0.1, 0.9)), sol(0.8, 0.8, 0.8))
        return t, t
    made = {n: s.ImageTexture(a) for n, a in images().items()}
    made["cyan"] = s.ImageTexture(None)          # the reference's "no data" image beside real ones
    noise = s.NoiseTexture(4.0, Rng(1984, 0))
    if name == "noise":
        return noise, noise
    if name == "chk_img_noise":                  # needs_uv has to be found THROUGH the checker
        return s.CheckerTexture(0.6, made["img256x128"], noise), s.CheckerTexture(0.6, noise, sol(0.8, 0.8, 0.8))
    return made[name], None


def carrier_world(texture, world, media=True, tree=False):
    """One texture on every carrier: sphere, negative-radius sphere inside a glass one, moving sphere, quads with all three
    normal axes in both windings (the AAQuad shortcuts) and a slanted one, a wall that reaches beyond +-256 and far into
    negative coordinates (Perlin's & 255 wrap, negative checker cells), a plain MakeBox, a box under Translate(RotateY(..)),
    a sphere under RotateY(Translate(..)), a DiffuseLight, and the phase functions of two media (sphere and box boundary;
    see make_texture for which texture they get).  The two small quads in the planes z = 0 and x = 4 lie on cell
    boundaries of the checkers (inverse scales 2 and 0.5): floor of +-0 and of an exact integer.  They are small, and no
    other surface of these scenes lies on a cell boundary of its checker, because the fast build contracts o + t * d into an
    fma, which lands on the other side of such a plane as often as not (measured with the far wall at z = -300: 13 % of
    the fast build's pixels off, none of the strict build's).
    `tree`: one object among the world's items that ObjectRec cannot express (SCENE_HAS_TREES: the nested kernels) --
    'bvh_object', a BvhNode over composites, or 'instance_of_list', Translate(RotateY(HittableList of composites))."""
    def build(s, Rng):
        tex, phase = make_texture(s, Rng, texture)
        lam, light = s.Lambertian(tex), s.DiffuseLight(tex)
        glass, grey = s.Dielectric(1.5), s.Lambertian((0.5, 0.5, 0.5))
        items = [
            s.Sphere((-6.0, 1.0, 0.0), 1.0, lam),
            s.Sphere((-3.5, 1.0, 0.5), 1.0, glass), s.Sphere((-3.5, 1.0, 0.5), -0.85, lam),
            s.MovingSphere((-1.0, 0.9, 0.0), (-1.0, 1.3, 0.0), 0.0, 1.0, 0.9, lam),
            s.Quad((0.3, 0.0, 0.1), (1.6, 0, 0), (0, 1.6, 0), lam), s.Quad((0.3, 1.8, 0.1), (0, 1.6, 0), (1.6, 0, 0), lam),
            s.Quad((4.1, 0.0, -1.8), (0, 0, 1.8), (0, 1.6, 0), lam), s.Quad((4.1, 1.8, -1.8), (0, 1.6, 0), (0, 0, 1.8), lam),
            s.Quad((-2.4, 2.4, 0.0), (0.4, 0, 0), (0, 0.4, 0), lam), s.Quad((4.0, 4.0, -0.4), (0, 0, 0.4), (0, 0.4, 0), lam),   # on cell boundaries
            s.Quad((0.0, 0.02, 1.5), (1.8, 0, 0), (0, 0, 1.8), lam), s.Quad((2.0, 0.02, 1.5), (0, 0, 1.8), (1.8, 0, 0), lam),
            s.Quad((2.1, 0.3, 0.2), (1.7, 0.3, 0.1), (0.2, 1.5, -0.4), lam),
            s.Quad((-400.0, -20.0, -300.3), (800, 0, 0), (0, 330, 0), lam),
            s.MakeBox((5.05, 0.0, 0.05), (6.45, 1.3, 1.45), lam),
            s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.2, 1.7, 1.2), lam), 30.0), (-6.5, 0.0, 2.5)),
            s.RotateY(s.Translate(s.Sphere((0, 0, 0), 0.7, lam), (-2.0, 0.7, 3.2)), -20.0),
            s.Sphere((-1.0, 3.6, 0.0), 0.8, light),
            s.Sphere((0, -1000, 0), 1000.0, grey)]
        if media and phase is not None:
            items.append(s.ConstantMedium(s.Sphere((-4.5, 3.4, 0.0), 1.0, glass), 1.5, phase))
            items.append(s.ConstantMedium(s.MakeBox((2.5, 2.4, -0.5), (4.3, 3.8, 0.9), glass), 2.0, phase))
        if tree:
            fog = s.ConstantMedium(s.Sphere((5.5, 3.0, 0.0), 0.8, glass), 1.2, phase) if phase is not None else \
                s.ConstantMedium(s.Sphere((5.5, 3.0, 0.0), 0.8, glass), 1.2, (0.8, 0.3, 0.2))
            members = [fog, s.MakeBox((6.65, 0.0, -1.45), (7.6, 1.05, -0.45), lam), s.Translate(s.Sphere((0, 0, 0), 0.7, lam), (7.0, 2.2, 0.0))]
            items.append(s.BvhNode(members) if tree == "bvh_object" else
                         s.Translate(s.RotateY(s.HittableList(members), 10.0), (0.0, 0.0, 0.3)))
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((-3.0, 4.0, 13.0), (0.3, 1.4, 0.0), (0, 1, 0), 42.0, W / H, 0.03, 13.0, 0.0, 1.0, (0.5, 0.6, 0.8))
        s.Commit()
    return build


def expected_kind(texture, world, media=True):
    """dispatch() of render.hip: a rich scene runs the general kernels (BVH 7, list 15).  The checker of two solids is not
    rich: BVH with media 6, BVH with instances 2 (19 leaves: walked, not scanned), list with instances 10; a list world
    with a medium always runs the general list kernel."""
    if texture not in PLAIN:
        return 7 if world == "bvh" else 15
    if world == "bvh":
        return 6 if media else 2
    return 15 if media else 10


def about(texture, media=True):
    """The counters of the oracle that a scene is about: each at least 5 % of its rays (no test passes vacuously)."""
    keys = []
    if texture in READS_UV:
        keys.append("image_lookups")
    if texture in ("noise", "chk_img_noise"):
        keys.append("noise_calls")
    if media and (texture not in READS_UV or texture == "chk_img_noise"):
        keys.append("medium_draws")
    return keys


def check(build, kind, min_exact, w=W, h=H, spp=4, counters=(), variants=(0, 1), label="", **render_kw):
    """test_custom_scenes_gpu.check with the kernel's identity and the oracle's counters pinned."""
    prod, orc = build_both(build)
    want, stats = orc.render(w, h, spp, want_stats=True, depth=render_kw.get("max_depth", 50))
    print(f"{label}: oracle rays {stats['rays']}, noise {stats['noise_calls']}, image {stats['image_lookups']}, "
          f"medium draws {stats['medium_draws']}")
    for key in counters:
        assert stats[key] >= 0.05 * stats["rays"], (key, stats[key], stats["rays"])
    frames = {}
    for variant in variants:
        got, st = prod.render(w, h, spp, variant=variant, **render_kw)
        exact, within, worst = compare(got, want)
        print(f"{label} variant {variant}: kernel kind {st.kernel_kind}, vgprs {st.kernel_vgprs}, lds {st.lds_bytes}, "
              f"bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
        assert st.kernel_kind == kind, (st.kernel_kind, kind)
        assert np.isfinite(got).all()
        if variant == 0:
            assert st.rays == stats["rays"], "ray counter differs from the oracle's RayColor iterations"
            assert within >= 0.999 and exact >= min_exact
        else:
            assert within >= 0.995
        frames[variant] = (got, st)
    return want, frames


# ------------------------------------------------------------------------------------------------------------------
# part 1: texture x carrier against the oracle
# ------------------------------------------------------------------------------------------------------------------
# Bit-exact share of the strict build against the oracle, measured on the MI355X (the comment), floor one to two points
# below.  Scenes without noise and media are expected to be bit-equal (floor 1.0; measured 1.0000 in both builds).  Device
# sin / log / acos differ from glibc's by an ulp: marble and media cost a few pixels.
CARRIER_FLOOR = {
    #                  (list world, bvh world)
    "img1x1": (1.0, 1.0),
    "img2x3": (1.0, 1.0),
    "img37x19": (1.0, 1.0),
    "img256x128": (1.0, 1.0),
    "cyan": (1.0, 1.0),
    "noise": (0.965, 0.965),          # 0.9811, 0.9810: marble on every carrier
    "chk_solid": (0.985, 0.985),      # 1.0000, 1.0000 (two media: device log)
    "chk_chk": (0.985, 0.985),        # 1.0000, 1.0000 (two media)
    "chk_img_noise": (0.975, 0.975),  # 0.9901, 0.9901
}


@pytest.mark.parametrize("world", ["list", "bvh"])
@pytest.mark.parametrize("texture", TEXTURES)
def test_texture_on_every_carrier_matches_the_oracle(texture, world):
    """Paths reached here that nothing else executes: quad u, v (make_surface; read only by an image texture); image texture on a
    moving sphere, on a box face (MakeBox leaf / BoxRec) and inside Translate / RotateY (uv in object space, p in world
    space); more than one image (ImageRec.offset != 0), images 1 x 1 / non-square / odd widths, the cyan "no data" image
    beside real ones; nested checkers (checker of checker, checker of image / noise: texture_value's table walk, needs_uv
    found through a checker child); DiffuseLight / Isotropic / ConstantMedium with a non-solid texture; negative radius
    (inv_r < 0) under a textured material.  Strict and fast build against the oracle."""
    floor = CARRIER_FLOOR[texture][world == "bvh"]
    check(carrier_world(texture, world), expected_kind(texture, world), floor, counters=about(texture),
          label=f"carriers {texture} {world}")


@pytest.mark.parametrize("texture", TEXTURES)
def test_textured_carriers_bvh_world_equals_list_world_bitwise(texture):
    """The reference's BVH = list invariant on the textured carriers without the two media (media draw random numbers per
    visit, and the two worlds visit them in different orders)."""
    import raytracinginoneweekendincuda_amd as rt
    frames = {}
    for world in ("list", "bvh"):
        prod = rt.Scene()
        carrier_world(texture, world, media=False)(prod, rt.Rng)
        frames[world] = prod.render(W, H, 4, variant=0)
        assert frames[world][1].kernel_kind == expected_kind(texture, world, media=False), frames[world][1].kernel_kind
    assert frames["list"][1].rays == frames["bvh"][1].rays
    assert np.array_equal(bits(frames["list"][0]), bits(frames["bvh"][0]))


# ------------------------------------------------------------------------------------------------------------------
# part 2: the rich kernels against each other
# ------------------------------------------------------------------------------------------------------------------
def deep_rich_world(n_noise=2, unused_noise=0, filler_boxes=0):
    """A world deep enough for the deep kernels (n_world_nodes > 64: the 64-box field of
    test_custom_scenes_gpu._deep_media_world) whose boxes, spheres, instances and media carry images, marble, and checkers
    plain and nested.  `n_noise` Perlin tables are in use (the second one on visible surfaces: boxes, a light, an
    instance); `unused_noise` more are created after everything else and never referenced -- they change no pixel, only
    FlatScene::n_perlin and with it whether the tables fit the deep kernels' LDS budget of 2 * sizeof(PerlinRec).
    `filler_boxes`: that many more small boxes behind the field, for the test that needs more than 64 KB of staged rows."""
    def build(s, Rng):
        rng = Rng(7)
        u = rng.uniform
        sol = lambda *c: s.SolidColor(c)
        img = {n: s.ImageTexture(a) for n, a in images().items()}
        noises = [s.NoiseTexture(sc, Rng(1984, k)) for k, sc in enumerate((4.0, 0.7)[:n_noise])]
        n0, n1 = noises[0], noises[-1]
        chk = s.CheckerTexture(0.5, sol(0.9, 0.1, 0.1), sol(0.1, 0.1, 0.9))
        chk_chk = s.CheckerTexture(2.0, chk, sol(0.8, 0.8, 0.8))
        chk_img = s.CheckerTexture(0.6, img["img256x128"], n0)
        glass = s.Dielectric(1.5)
        field = [s.Lambertian((0.4, 0.45, 0.4)), s.Lambertian(n1), s.Lambertian(chk), s.Lambertian(img["img37x19"]),
                 s.Lambertian(chk_img)]
        items = []
        for i in range(8):
            for k in range(8):
                x0, z0, h = -8.0 + 2.0 * i, -8.0 + 2.0 * k, 0.2 + 1.1 * u()
                items.append(s.MakeBox((x0, -1.0, z0), (x0 + 1.9, -1.0 + h, z0 + 1.9), field[(3 * i + k) % 5]))
        for k in range(filler_boxes):
            x0, z0 = -10.0 + 0.5 * (k % 40), -9.0 - 0.5 * (k // 40)
            items.append(s.MakeBox((x0, -1.0, z0), (x0 + 0.4, -0.2 + 0.1 * (k % 7), z0 + 0.4), field[k % 5]))
        mats = [s.Lambertian(img["img256x128"]), s.Metal((0.8, 0.8, 0.9), 0.1), glass, s.DiffuseLight(n1), s.Lambertian(chk_chk)]
        for k in range(16):
            items.append(s.Sphere((-7.0 + 0.95 * k, 0.8 + 0.6 * u(), -6.0 + 12.0 * u()), 0.3 + 0.25 * u(), mats[k % 5]))
        items.append(s.MovingSphere((3.0, 1.5, 1.0), (3.0, 2.0, 1.0), 0.0, 1.0, 0.5, s.Lambertian(img["img2x3"])))
        items.append(s.Quad((-4.0, 6.0, -4.0), (8.0, 0, 0), (0, 0, 8.0), s.DiffuseLight(chk)))
        items.append(s.Quad((-8.0, -1.0, -8.2), (16.0, 0, 0), (0, 5.0, 0), s.Lambertian(img["img37x19"])))
        inst = [s.Lambertian(n1), s.Lambertian(img["img256x128"]), s.Lambertian(chk_chk), s.Lambertian(n0)]
        for k in range(4):
            box = s.MakeBox((0, 0, 0), (0.9, 1.6 + 0.3 * k, 0.9), inst[k])
            items.append(s.Translate(s.RotateY(box, 15.0 + 20.0 * k), (-5.0 + 3.0 * k, 0.4, 4.0 - 2.5 * k)))
        marble = s.Lambertian(n0)   # one row: the deep kernels stage at most 4 KB of material rows
        cluster = [s.Sphere((1.6 * u(), 1.6 * u(), 1.6 * u()), 0.12, marble) for _ in range(40)]
        items.append(s.Translate(s.RotateY(s.HittableList(cluster), 15.0), (-1.0, 1.2, 3.0)))
        # media; their phase textures ignore u, v (make_texture)
        items.append(s.ConstantMedium(s.Sphere((0, 0, 0), 60.0, glass), 0.004, (1, 1, 1)))
        ball = s.Sphere((0.5, 1.4, 0.0), 1.0, glass)
        items.append(ball)
        items.append(s.ConstantMedium(ball, 0.6, n0))
        crate = s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.5, 1.5, 1.5), glass), -18.0), (-4.0, 0.6, -1.0))
        items.append(s.ConstantMedium(crate, 0.9, chk_chk))
        for k in range(unused_noise):
            s.NoiseTexture(11.0, Rng(1984, 2 + k))
        s.SetWorld(s.BvhNode(items))
        s.Camera((12.0, 6.0, 14.0), (0.0, 0.5, 0.0), (0, 1, 0), 38.0, W / H, 0.05, 18.0, 0.0, 1.0, (0.35, 0.45, 0.7))
        s.Commit()
    return build


DEEP_W, DEEP_H, DEEP_SPP = 64, 32, 6
DEEP_FLOOR = 0.98   # measured on the MI355X: 0.9971 with one Perlin table, 0.9956 with two


def _is_deep_kernel(st):
    """The 768-thread deep kernels keep every table in LDS and are compiled for at most 168 VGPRs; the two-wave general
    kernel has more registers and stages only what fits 52 KB (test_deep_kernel_falls_back_when_its_tables_do_not_fit)."""
    return st.kernel_vgprs <= 168


@pytest.mark.parametrize("n_noise", [1, 2])
def test_deep_rich_kernels_agree_bit_for_bit(n_noise):
    """Covers: two Perlin tables (table != 0 in perlin_turb, LDS offset table * sizeof(PerlinRec)); image / nested checker /
    marble on box faces, instances and media in the deep kernels.  The same picture through the segmented walk (kind
    263) and the deep reference-order kernel (RT_FLAG_REFERENCE_TREE: kind 7, tables in LDS), in both builds, and the
    strict one against the oracle."""
    prod, orc = build_both(deep_rich_world(n_noise))
    assert prod.info()["n_perlin"] == n_noise
    want, stats = orc.render(DEEP_W, DEEP_H, DEEP_SPP, want_stats=True)
    for key in ("image_lookups", "noise_calls", "medium_draws"):
        assert stats[key] >= 0.05 * stats["rays"], (key, stats[key], stats["rays"])
    for variant in (0, 1):
        seg, st = prod.render(DEEP_W, DEEP_H, DEEP_SPP, variant=variant)
        ref, st_ref = prod.render(DEEP_W, DEEP_H, DEEP_SPP, variant=variant, flags=FLAG_REFERENCE_TREE)
        assert st.kernel_kind == 263 and _is_deep_kernel(st), (st.kernel_kind, st.kernel_vgprs)
        assert st_ref.kernel_kind == 7 and _is_deep_kernel(st_ref), (st_ref.kernel_kind, st_ref.kernel_vgprs, st_ref.lds_bytes)
        assert st.rays == st_ref.rays
        assert np.array_equal(bits(seg), bits(ref)), variant
        if variant == 0:
            exact, within, worst = compare(seg, want)
            print(f"deep rich, {n_noise} tables: bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
            assert st.rays == stats["rays"] and within >= 0.999 and exact >= DEEP_FLOOR


def test_deep_rich_three_perlin_tables_read_from_global_memory_give_the_same_frame():
    """Covers: three Perlin tables.  The LDS budget is 2 * sizeof(PerlinRec), so with a third (unused) NoiseTexture the deep
    kernels stop fitting and the general kernel (kind 7, more than 168 VGPRs, small lds_bytes) reads Perlin through
    perlin_noise from global memory -- a second implementation of the sum that perlin_noise_lds computes in the deep
    kernels.  Strict build: frame, ray count and the continued RNG streams equal the two-table scene's bit for bit.
    The fast build contracts multiply-adds as the compiler sees fit in each instantiation, and the deep kernels and the
    two-wave general kernel are different instantiations: measured on this scene at 8 spp, 41592 rays through the
    segmented walk against 41466 through the general kernel.  A flipped decision inside the mist shifts the pixel's stream
    (C5 in the fast build is within 1e-5 of the oracle in 0.24 - 0.75 of its pixels), so neither
    frame is the reference of the other and neither meets the oracle's: measured within 0.9385 for the general kernel.  In
    the fast build the test therefore holds the general kernel only to itself: with and without RT_FLAG_REFERENCE_TREE,
    and 3 + 5 samples continued from its saved streams against 8 at once."""
    import raytracinginoneweekendincuda_amd as rt
    two, _ = build_both(deep_rich_world(2))
    three, orc = build_both(deep_rich_world(2, unused_noise=1))
    assert two.info()["n_perlin"] == 2 and three.info()["n_perlin"] == 3
    want, stats = orc.render(DEEP_W, DEEP_H, 8, want_stats=True)
    for variant in (0, 1):
        a, st_a = two.render(DEEP_W, DEEP_H, 8, variant=variant)
        assert st_a.kernel_kind == 263 and _is_deep_kernel(st_a)
        general = []
        for flags in (0, FLAG_REFERENCE_TREE):
            b, st_b = three.render(DEEP_W, DEEP_H, 8, variant=variant, flags=flags)
            exact, within, worst = compare(b, want)
            print(f"three tables, variant {variant}, flags {flags}: kind {st_b.kernel_kind}, vgprs {st_b.kernel_vgprs}, lds {st_b.lds_bytes}, "
                  f"rays {st_b.rays} (two tables {st_a.rays}, oracle {stats['rays']}), bit-exact {exact:.4f}, within {within:.4f}")
            assert st_b.kernel_kind == 7 and not _is_deep_kernel(st_b) and st_b.lds_bytes < 32 * 1024, (st_b.kernel_kind, st_b.kernel_vgprs, st_b.lds_bytes)
            general.append((b, st_b))
            if variant == 0:
                assert st_a.rays == st_b.rays
                assert np.array_equal(bits(a), bits(b)), flags
            assert np.isfinite(b).all()
        assert general[0][1].rays == general[1][1].rays and np.array_equal(bits(general[0][0]), bits(general[1][0]))
        exact, within, worst = compare(a, want)
        print(f"deep rich, two tables, variant {variant}: rays {st_a.rays}, bit-exact {exact:.4f}, within {within:.4f}")
        if variant == 0:
            assert st_a.rays == stats["rays"] and within >= 0.999 and exact >= DEEP_FLOOR
        # 3 + 5 samples from saved streams against 8 at once; in the strict build the first part by the LDS kernel of one
        # scene and the second by the global-memory kernel of the other
        film = rt.Film(DEEP_W, DEEP_H)
        film.render(two if variant == 0 else three, 3, variant=variant, flags=FLAG_ACCUMULATE)
        film.render(three, 5, variant=variant, flags=FLAG_ACCUMULATE | FLAG_KEEP_RNG_STATE)
        assert np.array_equal(bits(film.download()), bits(general[0][0])), variant


@pytest.mark.parametrize("batch", [1, 64])
def test_deep_rich_shading_batch_does_not_change_results(batch):
    """shade_batch reorders which lanes shade together (textures and media included); no bit may change."""
    import raytracinginoneweekendincuda_amd as rt
    prod = rt.Scene()
    deep_rich_world(2)(prod, rt.Rng)
    for flags, kind in ((0, 263), (FLAG_REFERENCE_TREE, 7)):
        a, st_a = prod.render(DEEP_W, DEEP_H, DEEP_SPP, variant=0, flags=flags)
        b, st_b = prod.render(DEEP_W, DEEP_H, DEEP_SPP, variant=0, flags=flags, shade_batch=batch)
        assert st_a.kernel_kind == st_b.kernel_kind == kind
        assert st_a.rays == st_b.rays and np.array_equal(bits(a), bits(b)), (batch, flags)


def test_deep_rich_pixel_classes_do_not_change_results():
    """The deep kernels serve heavy and light pixels by wave on films of at most seven generations of pixels per lane, at 64
    samples per pixel or more and 65536 pixels or more, when the kernel is the one with more than 64 KB of staged rows
    (device_scene.cpp deep_kernel / deep_roles / split): 200 more boxes bring the rows there, 256 x 256 x 64 turns the
    classes on, RT_FLAG_NO_PIXEL_CLASSES off.  Same frame, rays and saved streams either way, textured media included."""
    import raytracinginoneweekendincuda_amd as rt
    prod = rt.Scene()
    deep_rich_world(2, filler_boxes=200)(prod, rt.Rng)
    w = h = 256
    for flags, kind in ((0, 263), (FLAG_REFERENCE_TREE, 7)):
        a, b = rt.Film(w, h), rt.Film(w, h)
        st_a = a.render(prod, 64, variant=0, flags=flags)
        st_b = b.render(prod, 64, variant=0, flags=flags | FLAG_NO_PIXEL_CLASSES)
        print(f"pixel classes, flags {flags}: kind {st_a.kernel_kind}, vgprs {st_a.kernel_vgprs}, lds {st_a.lds_bytes}, rays {st_a.rays}")
        assert st_a.kernel_kind == st_b.kernel_kind == kind and _is_deep_kernel(st_a) and st_a.lds_bytes > 64 * 1024
        assert st_a.rays == st_b.rays
        assert np.array_equal(bits(a.download()), bits(b.download())), flags
        st_a = a.render(prod, 2, variant=0, flags=flags | FLAG_KEEP_RNG_STATE)
        st_b = b.render(prod, 2, variant=0, flags=flags | FLAG_KEEP_RNG_STATE | FLAG_NO_PIXEL_CLASSES)
        assert st_a.rays == st_b.rays
        assert np.array_equal(bits(a.download()), bits(b.download())), flags


# measured on the MI355X: 1.0000 / 1.0000 / 0.9891 - 0.9894 (every one of these scenes holds a medium)
NESTED_FLOOR = {"img37x19": 0.985, "chk_chk": 0.985, "chk_img_noise": 0.975}


@pytest.mark.parametrize("world", ["list", "bvh"])
@pytest.mark.parametrize("tree", ["bvh_object", "instance_of_list"])
@pytest.mark.parametrize("texture", sorted(NESTED_FLOOR))
def test_nested_kernels_shade_textured_carriers_like_the_oracle(texture, tree, world):
    """The carriers of part 1 with one object among the world's items that only the tree interpreter expresses
    (SCENE_HAS_TREES): the nested instantiations (kernel kinds with bit 32) take the hit's transforms from the winning
    tree node's chain.  Kind 47 is the nested list kernel, 39 the nested BVH kernel.  A BvhNode OBJECT over composites
    among the leaves of a BvhNode world is walked by the reference as part of the world's own tree, so flatten_scene keeps
    that whole world as one tree in a list of one: kind 47 there too."""
    kind = 39 if (world == "bvh" and tree == "instance_of_list") else 47
    check(carrier_world(texture, world, tree=tree), kind, NESTED_FLOOR[texture], label=f"nested {texture} {tree} {world}")


# ------------------------------------------------------------------------------------------------------------------
# part 3: the non-rich kernels with inline textures
# ------------------------------------------------------------------------------------------------------------------
def inline_world(shape, world):
    """Solids and checkers of two solids only (lower_materials copies them into the material row: tex_inline 1 / 2), so
    SCENE_RICH_TEXTURES stays clear and the non-rich kernels render it.  The inline checker sits on the ground, on spheres
    at negative coordinates, on a DiffuseLight and, by `shape`, on quads, plain and instanced boxes and media:
      spheres    static spheres only           prims      + quads and a moving sphere
      instances  + boxes plain and instanced   media      + two media with checkered phase functions
    No flat surface lies on a cell boundary of its own checker (see carrier_world)."""
    def build(s, Rng):
        sol = lambda c: s.SolidColor(c)
        chk = lambda sc, a, b: s.CheckerTexture(sc, sol(a), sol(b))
        ground = s.Lambertian(chk(0.5, (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
        lamp = s.DiffuseLight(chk(0.25, (6.0, 5.0, 4.0), (0.5, 0.5, 2.0)))
        dots = s.Lambertian(chk(0.3, (0.9, 0.2, 0.2), (0.2, 0.2, 0.9)))
        metal, glass = s.Metal((0.8, 0.8, 0.9), 0.05), s.Dielectric(1.5)
        items = [s.Sphere((0, -1000, 0), 1000.0, ground), s.Sphere((0.0, 4.5, -1.0), 1.5, lamp)]
        for k in range(18):
            items.append(s.Sphere((-5.6 + 0.66 * k, 0.45, -2.5 + 0.9 * (k % 5)), 0.45, (dots, metal, dots, glass)[k % 4]))
        if shape != "spheres":
            items.append(s.Quad((-6.0, 0.0, -4.0), (12, 0, 0), (0, 3.5, 0), dots))
            items.append(s.Quad((-6.1, 0.0, 3.0), (0, 0, -7), (0, 3.0, 0), lamp))
            items.append(s.Quad((1.0, 0.01, 2.0), (0.3, 0, 1.5), (2.0, 0.4, 0.2), dots))
            items.append(s.MovingSphere((3.0, 1.6, 1.0), (3.0, 2.0, 1.0), 0.0, 1.0, 0.5, dots))
        if shape in ("instances", "media"):
            items.append(s.MakeBox((-5.0, 0.0, 1.55), (-3.8, 1.4, 2.75), dots))
            items.append(s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.0, 2.0, 1.0), dots), 25.0), (4.0, 0.0, -1.0)))
            items.append(s.Translate(s.RotateY(s.MakeBox((0, 0, 0), (1.0, 1.05, 1.0), lamp), -35.0), (-2.0, 0.0, 2.2)))
        if shape == "media":
            items.append(s.ConstantMedium(s.Sphere((1.5, 1.6, 0.5), 1.0, glass), 1.5, chk(0.3, (0.9, 0.8, 0.1), (0.1, 0.6, 0.3))))
            items.append(s.ConstantMedium(s.MakeBox((-3.0, 0.0, -1.0), (-1.6, 1.6, 0.4), glass), 2.0, chk(0.5, (0.9, 0.9, 0.9), (0.1, 0.1, 0.1))))
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((0.5, 2.6, 9.5), (0, 1.0, 0), (0, 1, 0), 45.0, W / H, 0.03, 9.5, 0.0, 1.0, (0.15, 0.2, 0.35))
        s.Commit()
    return build


# (shape, world, flags, pixels_per_wave) -> kernel kind, by dispatch(): sphere list 16; list of primitives 8, with
# instances 10, their grouped forms + 128; primitive BVH on the library's tree 64, on the reference's 0; BVH with instances
# 2, with media 6; a list world with a medium always runs the general list kernel (15, the rich instantiation).
INLINE_CASES = [
    ("spheres", "list", 0, 64, 16),
    ("spheres", "bvh", 0, 64, 64),
    ("spheres", "bvh", FLAG_REFERENCE_TREE, 64, 0),
    ("prims", "list", 0, 64, 8),
    ("prims", "list", 0, 16, 136), ("prims", "list", 0, 4, 136), ("prims", "list", 0, 1, 136),
    ("prims", "bvh", 0, 64, 64),
    ("prims", "bvh", FLAG_REFERENCE_TREE, 64, 0),
    ("instances", "list", 0, 64, 10),
    ("instances", "list", 0, 16, 138), ("instances", "list", 0, 4, 138), ("instances", "list", 0, 1, 138),
    ("instances", "bvh", 0, 64, 2),
    ("media", "bvh", 0, 64, 6),
    ("media", "list", 0, 64, 15),
]
INLINE_MEDIA_FLOOR = 0.985   # measured on the MI355X: 1.0000 in the BVH world and in the list world


@pytest.mark.parametrize("shape,world,flags,ppw,kind", INLINE_CASES)
def test_inline_textures_in_the_non_rich_kernels(shape, world, flags, ppw, kind):
    """Covers: inline checker (tex_inline == 2) on a DiffuseLight, on instanced boxes, at negative coordinates and on a
    medium's Isotropic phase function, in the non-rich kernels.  Against the oracle, which evaluates the checker through
    its texture tree, and against RT_FLAG_FORCE_GENERAL -- the rich instantiation reading the same material rows."""
    import raytracinginoneweekendincuda_amd as rt
    build = inline_world(shape, world)
    # without media nothing transcendental is evaluated: bit equality with the oracle
    floor = INLINE_MEDIA_FLOOR if shape == "media" else 1.0
    counters = ("medium_draws",) if shape == "media" else ()
    _, frames = check(build, kind, floor, spp=6, counters=counters, label=f"inline {shape} {world} flags {flags} ppw {ppw}",
                      flags=flags, pixels_per_wave=ppw)
    if not (shape == "media" and world == "list"):
        assert kind & 1 == 0, "a scene of solids and checkers of solids must not need the rich instantiation"
    prod = rt.Scene()
    build(prod, rt.Rng)
    for variant in (0, 1):
        got, st = frames[variant]
        gen, st_gen = prod.render(W, H, 6, variant=variant, flags=flags | FLAG_FORCE_GENERAL)
        assert st_gen.kernel_kind & 1, st_gen.kernel_kind
        assert st_gen.rays == st.rays
        assert np.array_equal(bits(gen), bits(got)), (shape, world, variant)


# ------------------------------------------------------------------------------------------------------------------
# part 4: material parameters at their edges
# ------------------------------------------------------------------------------------------------------------------
N_EDGE_SWAPS = 14


def edge_materials(s):
    """Dielectric 1.0, 1/1.5, 2.4, 1.5; Metal fuzz 5 (clamped to 1), 0, exactly 1, albedo (1,1,1) and (0,0,0); black
    Lambertian (throughput 0: the path and its RNG stream go on) and one with albedo above 1; a light that emits 0 and one
    of 40 (frame values above 1 before the PPM clamp)."""
    g = s.Dielectric(1.5)
    return g, [s.Dielectric(1.0), s.Dielectric(1 / 1.5), s.Dielectric(2.4), g, s.Metal((0.9, 0.9, 0.9), 5.0), s.Metal((1, 1, 1), 0.0),
               s.Metal((0.8, 0.6, 0.2), 1.0), s.Metal((0, 0, 0), 0.3), s.Lambertian((0, 0, 0)), s.Lambertian((1.5, 1.2, 1.0)),
               s.DiffuseLight((0, 0, 0)), s.DiffuseLight((40, 40, 40))]


def edges_world(scene, world, swap=None):
    """scene: 'static'  spheres only: twelve edge materials in two rows and a hollow glass ball (radius r and -0.9 r on one centre)
              'moving'  the same plus a hollow MovingSphere pair
              'inside'  'static' with the camera placed inside a glass sphere of radius 0.8
              'mixed'   the materials on spheres, quads and instanced boxes in turn
    swap = k: edge material k replaced by grey Lambertian (tests/test_shading_host.py: every material decides paths)."""
    def build(s, Rng):
        grey = s.Lambertian((0.5, 0.5, 0.5))
        ground = s.Lambertian(s.CheckerTexture(0.5, s.SolidColor((0.2, 0.3, 0.1)), s.SolidColor((0.9, 0.9, 0.9))))
        g, mats = edge_materials(s)
        cam = (0.0, 1.5, 6.0)
        items = []
        if scene == "mixed":
            items.append(s.Quad((-30, -0.013, -30), (60, 0, 0), (0, 0, 60), ground))   # not on a cell boundary of its checker (carrier_world)
        else:
            items.append(s.Sphere((0, -1000, 0), 1000.0, ground))
        for k, m in enumerate(mats):
            x, z = -3.3 + 1.1 * (k % 6), 0.0 + 1.3 * (k // 6)
            m = grey if swap == k else m
            if scene != "mixed" or k % 3 == 0:
                items.append(s.Sphere((x, 0.5, z), 0.5, m))
            elif k % 3 == 1:
                items.append(s.Translate(s.RotateY(s.MakeBox((-0.4, 0, -0.4), (0.4, 0.9, 0.4), m), 20.0 + 5 * k), (x, 0.0, z)))
            else:
                items.append(s.Quad((x - 0.45, 0.0, z), (0.9, 0, 0), (0.1, 1.0, -0.2), m))
        items.append(s.Sphere((0.0, 0.5, 0.0), -0.45, grey if swap == 12 else g))   # the twin of mats[3] at (0, 0.5, 0)
        if scene == "moving":
            items.append(s.MovingSphere((1.5, 1.8, 0.5), (1.5, 2.1, 0.5), 0.0, 1.0, 0.5, g))
            items.append(s.MovingSphere((1.5, 1.8, 0.5), (1.5, 2.1, 0.5), 0.0, 1.0, -0.45, grey if swap == 13 else g))
        if scene == "inside":
            items.append(s.Sphere(cam, 0.8, g))
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera(cam, (0, 0.5, 0.5), (0, 1, 0), 45.0, W / H, 0.02, 5.5, 0.0, 1.0)
        s.Commit()
    return build


# dispatch(): a list of static spheres is the sphere list (16); moving spheres take it to the list of primitives (8); with
# boxes under transforms the list with instances (10).  BVH worlds of at most 16 leaves within the scan-cost budget are
# SCANNED in leaf order by the list kernels (small worlds: the 14 / 15 leaves of 'static' / 'inside' run as kind 8, not 64);
# RT_FLAG_ALWAYS_WALK sends them through the library's tree (64).  'moving' has 16 leaves as well.
# 'mixed' has 14 leaves too, but its instanced boxes put the scan cost above the budget of 64 half sphere tests
# (FlatScene::scan_cost, RenderArgs::small_world): it is walked by the BVH kernel with instances (2) either way.
EDGE_KINDS = {("static", "list"): 16, ("static", "bvh"): 8, ("moving", "list"): 8, ("moving", "bvh"): 8,
              ("inside", "list"): 16, ("inside", "bvh"): 8, ("mixed", "list"): 10, ("mixed", "bvh"): 2}
EDGE_KINDS_WALKED = {"static": 64, "moving": 64, "inside": 64, "mixed": 2}


@pytest.mark.parametrize("world", ["list", "bvh"])
@pytest.mark.parametrize("scene", ["static", "moving", "inside", "mixed"])
def test_material_edges_equal_the_oracle_bit_for_bit(scene, world):
    """Covers: Dielectric with an index other than 1.5 (1.0, below 1, 2.4) and the camera starting inside glass; negative
    radius (the hollow glass sphere: inv_r negative, the sphere-list filter's reach from sqrt(fabs(r2))); Metal fuzz >= 1
    through the clamp, fuzz exactly 0 and 1, albedo 0 and > 1; black Lambertian; a light that emits 0.  No noise and no
    medium: the strict build equals the oracle bit for bit, ray counter included, at max_depth 50 and 3; BVH worlds also
    walked (RT_FLAG_ALWAYS_WALK) where the launcher would scan their few leaves."""
    prod, orc = build_both(edges_world(scene, world))
    for depth in (50, 3):
        want, stats = orc.render(W, H, 8, depth=depth, want_stats=True)
        for flags in ((0, FLAG_ALWAYS_WALK) if world == "bvh" else (0,)):
            got, st = prod.render(W, H, 8, max_depth=depth, variant=0, flags=flags)
            kind = EDGE_KINDS_WALKED[scene] if flags else EDGE_KINDS[scene, world]
            exact, within, worst = compare(got, want)
            print(f"edges {scene} {world} depth {depth} flags {flags}: kind {st.kernel_kind}, rays {st.rays} / {stats['rays']}, "
                  f"bit-exact {exact:.4f}, within {within:.4f}, max {got.max():.3g}")
            assert st.kernel_kind == kind, (st.kernel_kind, kind)
            assert np.isfinite(got).all()
            assert st.rays == stats["rays"]
            assert np.array_equal(bits(got), bits(want))
        fast, _ = prod.render(W, H, 8, max_depth=depth, variant=1)
        assert np.isfinite(fast).all() and compare(fast, want)[1] >= 0.995
    assert want.max() > 1.0, "the light of 40 must show"


@pytest.mark.parametrize("scene", ["static", "moving", "inside"])
def test_material_edges_through_every_scan_and_walk(scene):
    """The same frame through the exact scan, the fp64 filter, the cooperative scan, eight pixels per wave, the reference's
    tree, the general kernels, and as 3 + 5 samples continued from saved streams."""
    import raytracinginoneweekendincuda_amd as rt
    spp = 8
    for world in ("list", "bvh"):
        prod = rt.Scene()
        edges_world(scene, world)(prod, rt.Rng)
        for variant in (0, 1):
            base, st0 = prod.render(W, H, spp, variant=variant)
            assert st0.kernel_kind == EDGE_KINDS[scene, world]
            if world == "list":
                others = [dict(flags=FLAG_EXACT_SCAN), dict(flags=FLAG_FILTER_FP64), dict(coop_threshold=65),
                          dict(pixels_per_wave=8), dict(flags=FLAG_FORCE_GENERAL)]
            else:
                others = [dict(flags=FLAG_ALWAYS_WALK), dict(flags=FLAG_ALWAYS_WALK | FLAG_REFERENCE_TREE),
                          dict(flags=FLAG_FORCE_GENERAL), dict(flags=FLAG_ALWAYS_WALK | FLAG_FORCE_GENERAL), dict(pixels_per_wave=8)]
            kinds = []
            for kw in others:
                got, st = prod.render(W, H, spp, variant=variant, **kw)
                kinds.append(st.kernel_kind)
                assert st.rays == st0.rays, (scene, world, variant, kw)
                assert np.array_equal(bits(got), bits(base)), (scene, world, variant, kw)
            print(f"edges {scene} {world} variant {variant}: kinds {st0.kernel_kind} then {kinds}")
            if world == "bvh":   # library tree, reference tree, general BVH kernel twice, grouped scan of the leaves
                assert kinds == [64, 0, 7, 7, 136], kinds
            else:                # a sphere list keeps its kernel at any pixels_per_wave; the list of primitives deals leaves to lanes
                assert kinds == [st0.kernel_kind] * 3 + [16 if st0.kernel_kind == 16 else 136, 15], kinds
            film = rt.Film(W, H)
            film.render(prod, 3, variant=variant, flags=FLAG_ACCUMULATE)
            film.render(prod, 5, variant=variant, flags=FLAG_ACCUMULATE | FLAG_KEEP_RNG_STATE)
            assert np.array_equal(bits(film.download()), bits(base)), (scene, world, variant)
