"""Corner normals and texture coordinates of triangles on the GPU (include/rtow.h rt_triangle_attr): the shading normal of a
radially attributed icosahedron is the sphere's; the hit record is the numpy restatement (tests/vertex_attr_restated.py) bit for
bit; every product of the library -- features, ray queries, path steps, advances, radiance, frames, adaptive and light-sampling
films -- sees that one record; texture coordinates select the texel they name; and nothing without attributes moved.  Every ray
set is a few thousand rays, every frame at most 32 x 24 pixels."""
import functools

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
import film_direct_restated as fdr
from frame_helpers import compare
from query_helpers import bits, centre_rays, dot3
from test_parity_gpu import TOL
from test_path_step_gpu import fold
from test_radiance_gpu import camera_rays
from triangle_meshes import icosphere, lattice
from vertex_attr_restated import as_stored, corner_attributes, image_texel, rays_at_faces, shading_normal, texture_uv

pytestmark = pytest.mark.gpu

W, H = 32, 24
N = W * H
SEED = 1984
HIT_RECORD = ("t", "normal", "front_face", "material")
GEOMETRY = ("t", "leaf", "front_face")
IMAGE = (np.arange(48, dtype=np.uint8).reshape(4, 4, 3) * 5 + 7)   # 4 x 4 texels, every channel of every texel its own byte


def committed(s, world, lookfrom=(0.0, 0.0, 300.0), lookat=(0.0, 0.0, 0.0)):
    s.SetWorld(world)
    s.Camera(lookfrom, lookat, (0, 1, 0), 40.0, W / H, 0.0, 1.0)
    s.Commit()
    return s


def same(a, b, keys):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


# ---- 1. radial normals ----
RADIUS, CENTRE, ANGLE = 90.0, np.array((190.0, 90.0, 190.0)), 25.0


def icosahedron_scene(form, attributed):
    verts, faces = icosphere(0, RADIUS)
    s = rt.Scene()
    kw = dict(normals=verts / RADIUS) if attributed else {}
    grey = s.Lambertian((0.5, 0.5, 0.5))
    if form == "bvh":
        return committed(s, s.TriangleMesh(verts, faces, grey, **kw))
    if form == "list":
        return committed(s, s.HittableList(s.TriangleMesh(verts, faces, grey, return_triangles=True, **kw)[1]))
    return committed(s, s.HittableList([s.Translate(s.RotateY(s.TriangleMesh(verts, faces, grey, **kw), ANGLE), CENTRE)]))


def to_world(p, form, point):
    """R/Instance.h:137-147 RotateY forward, then Translate (for directions: the rotation alone)."""
    if form != "instance":
        return p
    st, ct = np.sin(np.radians(ANGLE)), np.cos(np.radians(ANGLE))
    q = np.stack([ct * p[:, 0] + st * p[:, 2], p[:, 1], -st * p[:, 0] + ct * p[:, 2]], axis=-1)
    return q + CENTRE if point else q


@pytest.mark.parametrize("form", ["bvh", "list", "instance"])
def test_radial_corner_normals_give_the_spheres_normal(form):
    """n_k = vertex_k / R makes the interpolated m the hit point over R, so unit(m) is the sphere's normal at the hit point --
    1.4e-15 at worst in the restatement on a CPU; 1e-12 leaves three orders for the instance's rotation and the device's sqrt.
    The flat twin is off by more than a degree on more than 99 % of these rays (asserted: 90 %)."""
    verts, faces = icosphere(0, RADIUS)
    o, d, _ = rays_at_faces(verts, faces, 100, np.random.default_rng(26), 2.5 * RADIUS)
    o, d = np.ascontiguousarray(to_world(o, form, True)), np.ascontiguousarray(to_world(d, form, False))
    smooth = icosahedron_scene(form, True).intersect(o, d, want=GEOMETRY + ("normal",))
    flat = icosahedron_scene(form, False).intersect(o, d, want=GEOMETRY + ("normal",))
    hit = np.isfinite(smooth["t"])
    assert hit.all() and (smooth["front_face"] == 1).all(), "every ray comes from outside and hits"
    assert same(smooth, flat, GEOMETRY), "the hit decision is the flat triangle's"
    p = o + smooth["t"][:, None] * d
    centre = CENTRE if form == "instance" else np.zeros(3)
    radial = p - centre
    want = radial / np.sqrt(dot3(radial, radial))[:, None]
    err = np.abs(smooth["normal"] - want).max()
    off = np.degrees(np.arccos(np.clip(dot3(flat["normal"], want), -1.0, 1.0)))
    print(f"{form}: {hit.sum()} hits, shading normal off the sphere's by {err:.3g} at worst; the flat normal by more than a degree on "
          f"{np.mean(off > 1.0):.4f} of the rays (median {np.median(off):.1f}, worst {off.max():.1f} degrees)")
    assert np.mean(off > 1.0) > 0.9, "these rays tell flat normals from smooth ones"
    assert err <= 1e-12


# ---- 2. the restatement, bit for bit ----
@functools.lru_cache(maxsize=None)
def random_mesh():
    """lattice(3) and icosphere(1, 0.5) above it, as one mesh, with random corner normals and texture coordinates through index
    arrays of their own (the normals' a permutation of the corners, the texture coordinates' random).  A corner normal is its face's
    geometric normal tilted by up to 60 degrees, of a length between 0.5 and 2; a fifth of them are tilted by 100 to 170 degrees
    instead, so that the interpolated normal points under the surface on part of the face and the fallback to the geometric
    normal runs: on 0.13 of the hits for these seeds, by the restatement alone with the aimed barycentrics (a CPU is enough for
    that), inside the 1 % .. 60 % that the test asserts of the real hits."""
    rng = np.random.default_rng(26)
    lat, lat_faces = lattice(3)
    ball, ball_faces = icosphere(1, 0.5)
    verts = np.concatenate([lat, ball + (1.5, 0.9, 1.5)])
    faces = np.concatenate([lat_faces, ball_faces + len(lat)]).astype(np.int32)
    a, b, c = (verts[faces[:, k]] for k in range(3))
    ng = np.cross(b - a, c - a)
    ng = np.repeat(ng / np.linalg.norm(ng, axis=1, keepdims=True), 3, axis=0)
    corners = 3 * len(faces)
    tilt = np.radians(np.where(rng.uniform(size=corners) < 0.2, rng.uniform(100.0, 170.0, corners), rng.uniform(0.0, 60.0, corners)))
    side = rng.normal(size=(corners, 3))
    side -= (side * ng).sum(axis=1, keepdims=True) * ng
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    table = rng.uniform(0.5, 2.0, corners)[:, None] * (np.cos(tilt)[:, None] * ng + np.sin(tilt)[:, None] * side)
    order = rng.permutation(corners)
    normals = np.empty_like(table)
    normals[order] = table
    normal_faces = order.reshape(-1, 3).astype(np.int32)
    texcoords = rng.uniform(-0.25, 1.25, size=(37, 2))
    texcoord_faces = rng.integers(0, 37, size=faces.shape).astype(np.int32)
    return verts, faces, normals, normal_faces, texcoords, texcoord_faces


def random_mesh_scene(world, attributed):
    verts, faces, normals, normal_faces, texcoords, texcoord_faces = random_mesh()
    s = rt.Scene()
    kw = dict(normals=normals, normal_faces=normal_faces, texcoords=texcoords, texcoord_faces=texcoord_faces) if attributed else {}
    root, tris = s.TriangleMesh(verts, faces, s.Lambertian((0.5, 0.5, 0.5)), return_triangles=True, **kw)
    return committed(s, root if world == "bvh" else s.HittableList(tris), (1.5, 4.0, 6.0), (1.5, 0.3, 1.5))


@pytest.mark.parametrize("world", ["list", "bvh"])
def test_normal_and_uv_equal_the_restatement_bit_for_bit(world):
    verts, faces, normals, normal_faces, texcoords, texcoord_faces = random_mesh()
    o, d, _ = rays_at_faces(verts, faces, 30, np.random.default_rng(27), 3.0, both_sides=True)
    want = GEOMETRY + ("normal", "uv")
    # which triangle a ray hits: the list world's leaf is the triangle's number (triangles_out is in input order)
    tri = random_mesh_scene("list", False).intersect(o, d, want=("leaf",))["leaf"]
    flat = random_mesh_scene(world, False).intersect(o, d, want=want)
    scene = random_mesh_scene(world, True)
    got = scene.intersect(o, d, want=want)
    hit = np.isfinite(flat["t"])
    assert hit.mean() > 0.95 and np.array_equal(hit, tri >= 0)
    assert same(got, flat, GEOMETRY), "the hit decision is the flat triangle's"
    alpha, beta = flat["uv"][hit, 0], flat["uv"][hit, 1]
    front = flat["front_face"][hit] != 0
    # (a ray from behind a face of the ball meets the ball's far side first, from outside: the back faces are the lattice's, 18 of
    # the 98 faces with every other ray from below -- 9 %)
    assert 0.05 < front.mean() < 0.95, "hits from both sides"
    normal, fallback = shading_normal(alpha, beta, flat["normal"][hit], front, corner_attributes(tri[hit], normals, normal_faces))
    uv = texture_uv(alpha, beta, corner_attributes(tri[hit], texcoords, texcoord_faces))
    print(f"{world}: {hit.sum()} hits, the fallback to the geometric normal on {fallback.mean():.3f} of them")
    assert 0.01 <= fallback.mean() <= 0.6
    assert not np.array_equal(bits(got["normal"][hit]), bits(flat["normal"][hit]))
    assert np.array_equal(bits(got["normal"][hit]), bits(as_stored(normal))), \
        f"{np.sum((bits(got['normal'][hit]) != bits(as_stored(normal))).any(axis=-1))} of {hit.sum()} normals differ"
    assert np.array_equal(bits(got["uv"][hit]), bits(uv)), f"{np.sum((bits(got['uv'][hit]) != bits(uv)).any(axis=-1))} of {hit.sum()} uv differ"
    assert (got["normal"][~hit] == 0).all() and (got["uv"][~hit] == 0).all()
    # the torch device call: the same kernel on the caller's tensors
    dev = scene.intersect(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), want=want)
    torch.cuda.synchronize()
    assert same({k: v.cpu().numpy() for k, v in dev.items()}, got, want)


# ---- 3. one hit record everywhere ----
def box_world(s, world="bvh"):
    """An open box x, y in [0, 4], z in [-4, 0] with a lamp under its ceiling, and in it four attributed meshes: a Lambertian
    icosphere, a metal icosahedron under RotateY + Translate, a picture (an ImageTexture over texture coordinates) on the back
    wall and a ConstantMedium inside an icosphere.  Every mesh has corner normals; the picture's are tilted off its plane."""
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    items = [s.Quad((4, 0, -4), (0, 4, 0), (0, 0, 4), green), s.Quad((0, 0, -4), (0, 4, 0), (0, 0, 4), red),
             s.Quad((1.2, 3.98, -2.8), (1.6, 0, 0), (0, 0, 1.6), s.DiffuseLight((9.0, 9.0, 9.0))),
             s.Quad((0, 0, -4), (4, 0, 0), (0, 0, 4), white), s.Quad((0, 4, -4), (4, 0, 0), (0, 0, 4), white),
             s.Quad((0, 0, -4), (4, 0, 0), (0, 4, 0), white)]
    ball, ball_faces = icosphere(1, 0.7)
    items.append(s.TriangleMesh(ball + (1.0, 0.7, -2.4), ball_faces, s.Lambertian((0.3, 0.5, 0.8)), normals=ball / 0.7))
    ico, ico_faces = icosphere(0, 0.6)
    mirror = s.TriangleMesh(ico, ico_faces, s.Metal((0.8, 0.85, 0.88), 0.0), normals=ico / 0.6)
    items.append(s.Translate(s.RotateY(mirror, 25.0), (2.9, 0.6, -1.4)))
    flat, flat_faces = lattice(2, 0.8)
    picture = np.stack([flat[:, 0] + 1.2, flat[:, 2] + 2.0, np.full(len(flat), -3.9)], axis=-1)
    rng = np.random.default_rng(3)
    tilted = np.array((0.0, 0.0, 1.0)) + rng.uniform(-0.4, 0.4, size=(len(flat), 3))
    items.append(s.TriangleMesh(picture, flat_faces, s.Lambertian(s.ImageTexture(IMAGE)), normals=tilted, texcoords=flat[:, [0, 2]] / 1.6))
    fog, fog_faces = icosphere(1, 0.5)
    items.append(s.ConstantMedium(s.TriangleMesh(fog + (2.2, 2.7, -1.6), fog_faces, white, normals=fog / 0.5), 1.5, (0.9, 0.9, 0.9)))
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((2.0, 2.0, 5.2), (2.0, 1.8, -2.0), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, (0.0, 0.0, 0.0))
    s.Commit()
    return s


@functools.lru_cache(maxsize=None)
def box(world="bvh"):
    return box_world(rt.Scene(), world)


@functools.lru_cache(maxsize=None)
def box_rays(world="bvh"):
    arrays = camera_rays(box(world))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def box_radiance(world="bvh"):
    o, d, tm, states = box_rays(world)
    out = box(world).radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, want=("radiance", "path_rays", "rng_state"))
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("world", ["bvh", "list"])
def test_features_and_steps_carry_the_ray_querys_hit_record(world):
    scene = box(world)
    assert scene.info()["n_attributed_triangles"] == 80 + 20 + 8 + 80
    o, d, _, _ = centre_rays(scene, W, H)
    query = scene.intersect(o, d, want=HIT_RECORD + ("albedo", "uv", "leaf"))
    kinds = set(np.unique(query["material"]).tolist())
    assert {0, 1, 4} <= kinds, f"Lambertian, metal and the medium are all in view ({kinds})"
    on_picture = (query["material"] == 0) & np.isin(query["albedo"], (1.0 / 255.0) * IMAGE.astype(np.float64)).all(axis=-1)
    assert on_picture.sum() >= 4, "the picture is in view"
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=SEED, variant=0)
    albedo, normal, depth = (p.reshape(N, -1) for p in film.features())
    assert np.array_equal(np.isfinite(query["t"]), depth[:, 0] > 0)
    assert np.array_equal(bits(query["normal"]), bits(normal)) and np.array_equal(bits(query["albedo"]), bits(albedo))
    # the world has a medium, whose test draws: the step and the query are seeded alike
    step = scene.path_step(o, d, seed=SEED, first_sequence=0, want=("status",) + HIT_RECORD)
    assert same(step, query, HIT_RECORD)
    # the flat twin of the smooth meshes would report other normals: on the Lambertian ball the normal is the sphere's
    on_ball = (query["albedo"] == (0.3, 0.5, 0.8)).all(axis=-1)
    radial = (o[on_ball] + query["t"][on_ball, None] * d[on_ball]) - (1.0, 0.7, -2.4)
    assert on_ball.sum() >= 10 and np.abs(query["normal"][on_ball] - radial / np.sqrt(dot3(radial, radial))[:, None]).max() <= 1e-9


@pytest.mark.parametrize("world", ["bvh", "list"])
def test_steps_advances_radiance_and_the_frame_are_one_computation(world):
    scene = box(world)
    o, d, tm, states = box_rays(world)
    want = box_radiance(world)
    assert want["path_rays"].max() > 2
    acc, steps, final = fold(scene, o, d, tm, states, 50, {"status": set(), "material": set()})
    assert np.array_equal(bits(acc), bits(want["radiance"])), f"{np.sum((bits(acc) != bits(want['radiance'])).any(axis=-1))} of {N} rays differ"
    assert np.array_equal(steps, want["path_rays"]) and np.array_equal(final, want["rng_state"])
    batch = rt.PathBatch(scene, *(torch.from_numpy(np.array(a)).cuda() for a in (o, d)), times=torch.from_numpy(np.array(tm)).cuda(),
                         rng_state=torch.from_numpy(np.array(states).view(np.int32)).cuda())
    got = batch.run(50)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want["radiance"]))
    film = rt.Film(W, H)
    st = film.render(scene, 1, max_depth=50, seed=SEED, variant=0)
    assert np.array_equal(bits(film.download().reshape(N, 3)), bits(np.sqrt(want["radiance"])))
    assert int(st.rays) == int(want["path_rays"].sum(dtype=np.uint64))


KERNEL_WORLDS = {"box": lambda: box("bvh"),                                  # media and an image: the general kernel whatever the flags
                 "scene 13": lambda: rt.builtin_scene(13, 0, W, H),          # attributed meshes under instances
                 "scene 13 list": lambda: rt.builtin_scene(13, 1, W, H),
                 "mesh": lambda: random_mesh_scene("bvh", True)}              # primitives only: the library's tree


@pytest.mark.parametrize("name", sorted(KERNEL_WORLDS))
def test_the_frame_does_not_depend_on_the_kernel(name):
    scene = KERNEL_WORLDS[name]()
    frames, kinds = [], []
    for flags in (0, rt.FLAG_FORCE_GENERAL, rt.FLAG_REFERENCE_TREE):
        frame, st = scene.render(W, H, 4, variant=0, flags=flags)
        frames.append(frame)
        kinds.append(int(st.kernel_kind))
    print(f"{name}: kernel kinds {kinds}")
    assert (kinds[0] != kinds[1]) == (name != "box"), "a specialised kernel and the general one"
    assert np.array_equal(bits(frames[0]), bits(frames[1])) and np.array_equal(bits(frames[0]), bits(frames[2]))
    assert frames[0].max() > 0
    # the fast build: tests/test_parity_gpu.py's tolerance for fast against strict
    fast, _ = scene.render(W, H, 4, variant=1)
    exact, within, worst = compare(fast, frames[0], TOL)
    print(f"fast against strict: bit-exact {exact:.4f}, within {within:.4f}, max |d| {worst:.3g}")
    assert within >= 0.995


PIXELS = tuple(int(k) for k in np.random.default_rng(5).choice(N, 16, replace=False))
RULE = (4, 2, 0.35)


def test_adaptive_and_light_sampling_films_equal_their_restatements_at_sixteen_pixels():
    scene = box("bvh")
    rows, cols = np.divmod(np.array(PIXELS), W)
    for direct in (None, "mis"):
        for rule in (None, RULE):
            spp = 8 if rule else 3
            want = fdr.Frame(scene, W, H, SEED, pixels=PIXELS).launch(spp, 6, 1, rule=rule, direct=direct is not None)
            film = rt.Film(W, H)
            if rule:
                film.set_adaptive(*rule)
            film.render(scene, spp, direct=direct, max_depth=6, seed=SEED, variant=0)
            got = film.download()
            assert np.array_equal(bits(got[rows, cols]), bits(want.pixels()[rows, cols])), (direct, rule)
            if rule:
                counts = film.sample_counts()[rows, cols]
                print(f"direct {direct}: samples at the sixteen pixels {sorted(counts.tolist())}")
                assert np.array_equal(counts, want.counts()[rows, cols])


# ---- 4. texture coordinates ----
@pytest.mark.parametrize("mapping", ["identity", "quarter turn"])
def test_texture_coordinates_select_the_texel(mapping):
    corners = np.array([(0.0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)])
    faces = np.array([(0, 1, 2), (0, 2, 3)], dtype=np.int32)
    tex = np.array([(0.0, 0), (1, 0), (1, 1), (0, 1)])
    if mapping == "quarter turn":
        tex = tex[[1, 2, 3, 0]]   # corner k shows what corner k + 1 showed: the picture turned by 90 degrees
    s = rt.Scene()
    root, tris = s.TriangleMesh(corners, faces, s.Lambertian(s.ImageTexture(IMAGE)), return_triangles=True, texcoords=tex)
    committed(s, s.HittableList(tris), (0.5, 0.5, 3.0), (0.5, 0.5, 0.0))
    flat = rt.Scene()
    committed(flat, flat.HittableList(flat.TriangleMesh(corners, faces, flat.Lambertian((0.5, 0.5, 0.5)), return_triangles=True)[1]))
    # rays at the centres of an 8 x 8 grid over the square: two by two inside every texel, none on the diagonal's texel borders
    g = (np.arange(8) + 0.5) / 8.0
    x, y = (a.ravel() for a in np.meshgrid(g + 0.01, g - 0.013))
    o = np.ascontiguousarray(np.stack([x, y, np.full(x.size, 2.0)], axis=-1))
    d = np.ascontiguousarray(np.broadcast_to((0.0, 0.0, -1.0), o.shape))
    twin = flat.intersect(o, d, want=("t", "uv", "leaf"))
    got = s.intersect(o, d, want=("t", "uv", "leaf", "albedo"))
    assert np.isfinite(got["t"]).all() and same(got, twin, ("t", "leaf"))
    uv = texture_uv(twin["uv"][:, 0], twin["uv"][:, 1], corner_attributes(twin["leaf"], tex, faces))
    assert np.array_equal(bits(got["uv"]), bits(uv))
    near_border = (np.abs(uv * 4 - np.round(uv * 4)) <= 1e-9).any(axis=-1)
    assert near_border.mean() <= 0.01 and not near_border.any(), "the rays are aimed inside the texels"
    want = image_texel(IMAGE, uv[:, 0], uv[:, 1])
    assert np.array_equal(bits(got["albedo"]), bits(as_stored(want)))
    assert len(np.unique(got["albedo"], axis=0)) == 16, "every texel is seen"
    # and the mapping is the one asked for: U, V of the identity are the point's x, y (alpha, beta and the five operations
    # behind them round values of at most 1: a few times 1.1e-16)
    if mapping == "identity":
        assert np.abs(uv - o[:, :2]).max() <= 1e-14
    else:
        assert np.abs(uv - np.stack([1.0 - o[:, 1], o[:, 0]], axis=-1)).max() <= 1e-14


# ---- 5. nothing else moved ----
def test_a_mesh_without_attributes_and_scene_thirteen_against_scene_twelve():
    twelve, thirteen = rt.builtin_scene(12, 0, W, H), rt.builtin_scene(13, 0, W, H)
    # scene 12's two meshes through TriangleMesh(..., normals=None, texcoords=None), in a copy of scene 12 built here
    def cornell(**kw):
        s = rt.Scene()
        white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
        items = [s.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green), s.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),
                 s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), s.DiffuseLight((15.0, 15.0, 15.0))),
                 s.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white), s.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white),
                 s.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)]
        v, f = icosphere(2, 100.0)
        items.append(s.Translate(s.TriangleMesh(v, f, white, **kw), (347.5, 100.0, 377.5)))
        v, f = icosphere(0, 90.0)
        items.append(s.Translate(s.RotateY(s.TriangleMesh(v, f, s.Metal((0.8, 0.85, 0.88), 0.0), **kw), -18.0), (212.5, 90.0, 147.5)))
        s.SetWorld(s.BvhNode(items))
        s.Camera((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 0.0, (0.0, 0.0, 0.0))
        s.Commit()
        return s

    plain, st_plain = cornell().render(W, H, 4, variant=0)
    none, st_none = cornell(normals=None, texcoords=None).render(W, H, 4, variant=0)
    assert np.array_equal(bits(plain), bits(none)) and st_plain.kernel_kind == st_none.kernel_kind and st_plain.rays == st_none.rays
    frame12, st12 = twelve.render(W, H, 4, variant=0)
    assert np.array_equal(twelve.dump_camera(), cornell().dump_camera())
    assert np.array_equal(bits(none), bits(frame12)) and st_none.kernel_kind == st12.kernel_kind, "scene 12's frame, bit for bit"
    frame13, st13 = thirteen.render(W, H, 4, variant=0)
    assert st12.kernel_kind == st13.kernel_kind
    assert not np.array_equal(bits(frame12), bits(frame13)), "scene 13 is shaded smoothly"
    o, d, _, _ = centre_rays(twelve, W, H)
    a = twelve.intersect(o, d, want=GEOMETRY + ("normal",))
    b = thirteen.intersect(o, d, want=GEOMETRY + ("normal",))
    assert same(a, b, GEOMETRY), "t, leaf and front_face planes"
    moved = (bits(a["normal"]) != bits(b["normal"])).any(axis=-1)
    on_mesh = np.isin(a["leaf"], np.flatnonzero(twelve.dump_leaves()[0] == 3))
    print(f"{moved.sum()} of {on_mesh.sum()} centre rays on the meshes report another normal")
    assert moved.sum() >= 20 and not moved[~on_mesh].any()
