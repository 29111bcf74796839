"""First-hit feature buffers (rt_film_render_features): geometry against closed forms, the albedo against the render path through
"emissive twins", and the plumbing around the pass (stripes, progressive frames, statistics, the executable)."""
import os
import subprocess

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from conftest import ROOT, build_both
from query_helpers import bits, centre_rays, mixed_world, sphere_roots
from test_custom_scenes_gpu import NESTINGS, _coincident

pytestmark = pytest.mark.gpu


def centre_ray_grid(scene, width, height):
    """query_helpers.centre_rays in the shape of the feature planes: (background, origin (3,), directions (H, W, 3))."""
    o, d, _, bg = centre_rays(scene, width, height)
    return bg, o[0], d.reshape(height, width, 3)


W, H = 32, 24


def features_of(scene, width=W, height=H, **kw):
    film = rt.Film(width, height)
    film.render_features(scene, **kw)
    return film.features()


# ---- D: geometry, samples = 0, pinhole camera ----
def test_sphere_depth_and_normal_equal_the_closed_form():
    bg_colour, centre, radius, colour = (0.2, 0.3, 0.9), (0.1, 0.05, -3.0), 0.8, (0.6, 0.4, 0.1)
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere(centre, radius, s.Lambertian(colour))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, bg_colour)
    s.Commit()
    bg, origin, d = centre_ray_grid(s, W, H)
    t, _, rel_disc = sphere_roots(origin, d, centre, radius)
    hit = (rel_disc > 0) & (t > 0.001)   # R/Sphere.h:28-60 over [0.001, inf) for rays from outside
    grazing = np.abs(rel_disc) <= 1e-9
    assert grazing.mean() <= 0.02, "the sphere was chosen so that (nearly) no centre ray grazes it"
    assert 0.1 < hit.mean() < 0.9
    for variant in (0, 1):
        albedo, normal, depth = features_of(s, samples=0, variant=variant)
        sure_hit, sure_miss = hit & ~grazing, ~hit & ~grazing
        want_depth = t * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        want_normal = ((origin + t[..., None] * d) - np.asarray(centre)) / radius
        rel = np.abs(depth[sure_hit] - want_depth[sure_hit]) / want_depth[sure_hit]
        err_n = np.abs(normal[sure_hit] - want_normal[sure_hit])
        print(f"variant {variant}: depth rel err {rel.max():.3g}, normal err {err_n.max():.3g}, {sure_hit.sum()} hits, {grazing.sum()} left out")
        assert rel.max() <= 1e-12 and err_n.max() <= 1e-12
        assert np.array_equal(albedo[sure_hit], np.broadcast_to(colour, albedo[sure_hit].shape))
        assert (depth[sure_miss] == 0).all() and (normal[sure_miss] == 0).all()
        assert np.array_equal(albedo[sure_miss], np.broadcast_to(bg, albedo[sure_miss].shape)), "a miss shows the background, exactly"


@pytest.mark.parametrize("world", ["bvh", "list"])
def test_quads_and_an_instanced_box_have_unit_normals_against_the_ray(world):
    floor_c, wall_c, box_c = (0.25, 0.5, 0.125), (0.5, 0.25, 0.75), (0.75, 0.75, 0.25)
    s = rt.Scene()
    items = [s.Quad((-30, -1, -30), (60, 0, 0), (0, 0, 60), s.Lambertian(floor_c)),
             s.Quad((-30, -1, -6), (60, 0, 0), (0, 30, 0), s.Metal(wall_c, 0.1)),
             s.RotateY(s.Translate(s.MakeBox((-0.6, -1.0, -0.6), (0.6, 0.4, 0.6), s.Lambertian(box_c)), (0.3, 0.0, -2.5)), 25.0)]
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0, 0.6, 3), (0, 0, -2), (0, 1, 0), 50.0, W / H, 0.0, 1.0)
    s.Commit()
    _, origin, d = centre_ray_grid(s, W, H)
    albedo, normal, depth = features_of(s, samples=0)
    hit = depth > 0
    assert hit.all(), "floor and wall fill the frame"
    assert np.abs(np.linalg.norm(normal, axis=-1) - 1.0).max() <= 1e-15
    assert ((normal * d).sum(axis=-1) < 0).all(), "face() turns the normal against the ray"
    on_floor, on_wall, on_box = ((albedo == c).all(axis=-1) for c in (floor_c, wall_c, box_c))
    assert on_floor.any() and on_wall.any() and on_box.sum() > 20 and (on_floor | on_wall | on_box).all()

    def plane_normal(u, v):   # R/Quad.h:33-37: unit_vector(cross(u, v)), v / t being (1 / t) * v
        n = np.cross(u, v).astype(np.float64)
        return (1.0 / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])) * n

    floor_n, wall_n = -plane_normal((60, 0, 0), (0, 0, 60)), plane_normal((60, 0, 0), (0, 30, 0))   # the camera is above / in front
    assert floor_n[1] > 0.99 and wall_n[2] > 0.99
    assert (normal[on_floor] == floor_n).all() and (normal[on_wall] == wall_n).all(), "the plane's normal, exactly"
    # the box's faces: the axes turned by -25 degrees about y (R/Instance.h:137-147), or straight up
    st, ct = np.sin(np.radians(25.0)), np.cos(np.radians(25.0))
    faces = np.array([(0, 1, 0), (ct, 0, -st), (-ct, 0, st), (st, 0, ct), (-st, 0, -ct)])
    assert np.abs(normal[on_box][:, None, :] - faces[None]).max(axis=-1).min(axis=-1).max() <= 1e-15


def test_dense_medium_reports_its_boundary_and_no_normal():
    phase, centre, radius = (0.125, 0.75, 0.375), (0.0, 0.0, -3.0), 1.0
    s = rt.Scene()
    fog = s.ConstantMedium(s.Sphere(centre, radius, s.Lambertian((0.5, 0.5, 0.5))), 1e9, phase)
    s.SetWorld(s.BvhNode([fog, s.Sphere((0, -101, -3), 100.0, s.Lambertian((0.5, 0.5, 0.5)))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 50.0, W / H, 0.0, 1.0)
    s.Commit()
    _, origin, d = centre_ray_grid(s, W, H)
    t, _, rel_disc = sphere_roots(origin, d, centre, radius)
    hit = (rel_disc > 0) & (t > 0.001)
    albedo, normal, depth = features_of(s, samples=0)
    in_fog = (albedo == phase).all(axis=-1)
    assert in_fog.sum() >= 1 and not (in_fog & ~hit).any()
    assert (normal[in_fog] == 0).all(), "a medium has no shading normal"
    boundary = (t * np.linalg.norm(d, axis=-1))[in_fog]
    assert np.abs(depth[in_fog] - boundary).max() <= 1e-6, "at density 1e9 the scattering point lies on the boundary"
    assert (np.linalg.norm(normal[~in_fog & (depth > 0)], axis=-1) > 0.99).all()


# ---- E: the emissive twin ----
class View:
    """A scene seen through a filter, for building one scene function several ways (rt.Scene and conftest.OracleScene alike):
    emissive = every material becomes a DiffuseLight over the texture the feature pass reports for it; no_media = a ConstantMedium
    is replaced by its boundary; lens = the camera gets this aperture and an open shutter whatever the function asked for."""

    def __init__(self, scene, emissive=False, no_media=False, lens=None):
        self._s, self._emissive, self._no_media, self._lens = scene, emissive, no_media, lens

    def __getattr__(self, name):
        return getattr(self._s, name)

    def Lambertian(self, c):
        return self._s.DiffuseLight(c) if self._emissive else self._s.Lambertian(c)

    def Isotropic(self, c):
        return self._s.DiffuseLight(c) if self._emissive else self._s.Isotropic(c)

    def Metal(self, c, fuzz):
        return self._s.DiffuseLight(self._s.SolidColor(c)) if self._emissive else self._s.Metal(c, fuzz)

    def Dielectric(self, ior):
        return self._s.DiffuseLight((1.0, 1.0, 1.0)) if self._emissive else self._s.Dielectric(ior)

    def ConstantMedium(self, boundary, density, c):
        return boundary if self._no_media else self._s.ConstantMedium(boundary, density, c)

    def Camera(self, lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=0.0, background=(0.70, 0.80, 1.00)):
        if self._lens is not None:
            aperture, time0, time1 = self._lens, 0.0, 1.0
        self._s.Camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, time0, time1, background)


TW, TH = 24, 16


# name -> (scene function, media replaced by their boundaries, a Perlin texture is in sight)
TWINS = {
    "mixed list": (lambda s, Rng: mixed_world(s, Rng, 1, TW / TH), False, True),
    "mixed bvh": (lambda s, Rng: mixed_world(s, Rng, 0, TW / TH), False, True),
    "many_chained_transforms": (NESTINGS["many_chained_transforms"], False, True),
    "instance_of_composites": (NESTINGS["instance_of_composites"], True, False),
    "bvh_inside_a_list_world": (NESTINGS["bvh_inside_a_list_world"], True, False),
    "instance_of_a_bvh_of_composites": (NESTINGS["instance_of_a_bvh_of_composites"], True, False),
    "coincident bvh": (_coincident(0), False, False),
    "coincident list": (_coincident(1), False, False),
}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_albedo_equals_the_render_of_the_emissive_twin(name):
    """The twin of a scene has every material replaced by a DiffuseLight over what the feature pass reports as that material's
    albedo (metal: SolidColor(albedo), glass: (1, 1, 1)).  Its paths end at the first hit and draw nothing but the camera's numbers,
    so render(twin, spp = N)^2 * N is the sum of the first hits' albedos in sample order: sqrt(features(original, samples = N).albedo)
    must equal it bit for bit -- seeding, camera draws, traversal order, tie rule, make_surface, textures and averaging are then
    those of the render path, which the oracle verifies (strict build: the twin's render against the oracle's, too).
    No scene here keeps a medium (a medium's twin would need an emissive phase function, which no constructor builds): the
    nestings that have some are built with each ConstantMedium replaced by its boundary, original and twin alike; every camera
    gets an aperture of 0.1 and the shutter 0..1."""
    build, no_media, perlin = TWINS[name]
    original = rt.Scene()
    build(View(original, no_media=no_media, lens=0.1), rt.Rng)
    twin, twin_oracle = build_both(lambda s, Rng: build(View(s, emissive=True, no_media=no_media, lens=0.1), Rng))
    for samples in (1, 4):
        want_oracle = twin_oracle.render(TW, TH, samples)
        for variant in (0, 1):
            albedo, normal, depth = features_of(original, TW, TH, samples=samples, variant=variant)
            rendered, st = twin.render(TW, TH, samples, variant=variant)
            same = float(np.mean(np.all(bits(np.sqrt(albedo)) == bits(rendered), axis=-1)))
            print(f"{name}, {samples} samples, variant {variant}: kernel kind {st.kernel_kind}, sqrt(albedo) == render(twin) on {same:.4f} of the pixels")
            assert np.array_equal(bits(np.sqrt(albedo)), bits(rendered))
            assert st.rays == TW * TH * samples, "a twin's path is its primary ray"
            if variant == 0:
                exact = float(np.mean(np.all(bits(rendered) == bits(want_oracle), axis=-1)))
                within = float(np.mean(np.all(np.abs(rendered - want_oracle) <= 1e-5, axis=-1)))
                print(f"    twin against the oracle: bit-exact {exact:.4f}, within 1e-5 {within:.4f}")
                assert within >= 0.999 and exact >= (0.94 if perlin else 1.0)   # (the marble floor of tests/test_parity_gpu.py)


# ---- F: plumbing ----
@pytest.mark.parametrize("world_size", [2, 3])
def test_striped_films_hold_the_single_films_features(world_size):
    width, height, stripe = 24, 20, 4
    scene = rt.builtin_scene(9, 0, width, height)   # the Book-2 final scene: media draw from the pixel's stream
    for samples in (0, 2):
        whole = features_of(scene, width, height, samples=samples)
        parts = [np.zeros_like(p) for p in whole]
        for rank in range(world_size):
            film = rt.Film(width, height, stripe_rows=stripe, rank=rank, world_size=world_size)
            film.render_features(scene, samples=samples)
            rows = rt.stripe_rows(height, stripe, rank, world_size)
            others = np.setdiff1d(np.arange(height), rows)
            for part, plane in zip(parts, film.features()):
                assert (plane[others] == 0).all(), "rows of other ranks are 0"
                part[rows] = plane[rows]
        for part, plane in zip(parts, whole):
            assert np.array_equal(bits(part), bits(plane))


def test_feature_pass_leaves_frames_statistics_and_rng_streams_alone():
    width, height = 24, 20
    scene = rt.builtin_scene(8, 0, width, height)   # Cornell smoke
    keep = rt.FLAG_KEEP_RNG_STATE | rt.FLAG_ACCUMULATE
    a, b = rt.Film(width, height), rt.Film(width, height)
    b.render_features(scene, samples=3, seed=7)
    sa, sb = a.render(scene, 2, variant=0, flags=keep), b.render(scene, 2, variant=0, flags=keep)
    assert (sa.kernel_kind, sa.rays, sa.samples, sa.lds_bytes) == (sb.kernel_kind, sb.rays, sb.samples, sb.lds_bytes)
    assert np.array_equal(bits(a.download()), bits(b.download())), "a plain render after a feature pass"
    before = b.features()
    b.render_features(scene, samples=1)   # between two launches of a progressive frame
    sa, sb = a.render(scene, 3, variant=0, flags=keep), b.render(scene, 3, variant=0, flags=keep)
    assert (sa.kernel_kind, sa.rays) == (sb.kernel_kind, sb.rays)
    assert np.array_equal(bits(a.download()), bits(b.download()))
    whole, _ = scene.render(width, height, 5, variant=0)
    assert np.array_equal(bits(b.download()), bits(whole))
    assert not np.array_equal(before[0], b.features()[0])


def _read_pfm(path):
    with open(path, "rb") as fp:
        assert fp.readline().strip() == b"PF"
        width, height = map(int, fp.readline().split())
        assert float(fp.readline()) < 0   # little-endian
        return np.frombuffer(fp.read(), dtype="<f4").reshape(height, width, 3)


def test_rtow_writes_what_the_api_computes(tmp_path):
    width, height, spp = 32, 24, 4
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    out, raw, prefix = tmp_path / "clean.ppm", tmp_path / "raw.ppm", tmp_path / "aov"
    subprocess.run([exe, "--scene", "7", "--width", str(width), "--height", str(height), "--spp", str(spp), "--variant", "strict",
                    "--denoise", "--denoise-iterations", "3", "--denoise-sigmas", "0.5,0.2,0.4,0.3", "--feature-samples", "2",
                    "--raw-output", str(raw), "--aov-prefix", str(prefix), "--output", str(out)], check=True, cwd=ROOT, timeout=120)
    scene = rt.builtin_scene(7, 0, width, height)
    film = rt.Film(width, height)
    film.render(scene, spp, variant=0, pixels_per_wave=0)
    film.render_features(scene, samples=2, variant=0)
    film.denoise(iterations=3, sigma_color=0.5, sigma_albedo=0.2, sigma_normal=0.4, sigma_depth=0.3)
    albedo, normal, depth = film.features()
    for suffix, plane in (("albedo", albedo), ("normal", normal), ("depth", np.repeat(depth[..., None], 3, axis=-1))):
        assert np.array_equal(_read_pfm(f"{prefix}_{suffix}.pfm"), plane.astype(np.float32)), suffix
    for path, frame in ((out, film.denoised()), (raw, film.download())):
        want = tmp_path / "want.ppm"
        rt.write_ppm(want, frame)
        assert open(path, "rb").read() == open(want, "rb").read(), path
