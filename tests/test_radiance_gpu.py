"""Radiance queries (rt_scene_radiance, Scene.radiance): whole paths for caller-supplied rays.  The keystone is the render itself:
the host restates every pixel's first camera ray and hands over the pixel's stream where the camera left it, and the square root
of the radiance that comes back is the rendered pixel, bit for bit.  Beside it closed forms that are exact in both builds, the
stream rules (seeding, chaining through the state, splitting, permuting), the plumbing (batch edges, outputs left out, the torch
path, the executable) and the strict build against the fast one.  Every ray set is at most 32 x 24 rays and 4 samples."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from raytracinginoneweekendincuda_amd import _lib, api
from conftest import ROOT
from query_helpers import bits, centre_rays, mixed_world, sphere_roots

pytestmark = pytest.mark.gpu

W, H = 32, 24
N = W * H
SEED = 1984
ALL = ("radiance", "path_rays", "rng_state")


def same(got, want, keys=ALL):
    return all(np.array_equal(bits(got[k]), bits(want[k])) for k in keys)


def frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- rays ----
def camera_rays(scene, seed=SEED, width=W, height=H):
    """The first camera ray of every pixel of a render with this seed, restated from dump_camera {bg, origin, llc, horizontal,
    vertical, u, v, w, lens radius, time0, time1} and rt.Rng(seed, j * W + i) in camera_ray's order of draws and operations (IEEE
    double, nothing fused on either side), and the pixel's stream after those draws.  Ray k = j * W + i.  Returns (origins (N, 3),
    directions (N, 3), times (N,), states (N, 6) uint32)."""
    cam = scene.dump_camera()
    origin, llc, hor, ver, cam_u, cam_v = (cam[3 * k:3 * k + 3] for k in (1, 2, 3, 4, 5, 6))
    lens_radius, time0, time1 = cam[24], cam[25], cam[26]
    n = width * height
    o, d, tm, states = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros((n, 6), dtype=np.uint32)
    for j in range(height):
        for i in range(width):
            k = j * width + i
            rng = rt.Rng(seed, k)
            u = np.float64(np.float32(i) + np.float32(rng.uniform())) / np.float64(width)   # int + float adds in fp32
            v = np.float64(np.float32(j) + np.float32(rng.uniform())) / np.float64(height)
            while True:
                a, b = np.float64(rng.uniform()), np.float64(rng.uniform())
                p = 2.0 * np.array([a, b, 0.0]) - np.array([1.0, 1.0, 0.0])
                if p[0] * p[0] + p[1] * p[1] + p[2] * p[2] < 1.0:
                    break
            rd = lens_radius * p
            offset = rd[0] * cam_u + rd[1] * cam_v
            tm[k] = time0 + np.float64(rng.uniform()) * (time1 - time0)
            o[k] = origin + offset
            d[k] = (((llc + u * hor) + v * ver) - origin) - offset
            states[k] = rng.state()
    return o, d, tm, states


def host_states(seed, first_sequence, count):
    return np.array([rt.Rng(seed, k + first_sequence).state() for k in range(count)], dtype=np.uint32)


# ---- scenes ----
SCENES = {
    "mixed bvh": lambda: mixed_world(rt.Scene(), rt.Rng, 0, W / H), "mixed list": lambda: mixed_world(rt.Scene(), rt.Rng, 1, W / H),
    "scene 9 bvh": lambda: rt.builtin_scene(9, 0, W, H), "scene 9 list": lambda: rt.builtin_scene(9, 1, W, H),   # media, boxes, earth, Perlin
    "scene 7 bvh": lambda: rt.builtin_scene(7, 0, W, H),
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def rays_of(name):
    """The camera rays of the scene's 1-spp render with their streams, computed once and shared (nobody writes to them)."""
    arrays = camera_rays(scene_of(name))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def render_of(name, variant=0):
    """The 1-spp frame of the parent's render kernels, as rays: (pixels (N, 3), stats.rays)."""
    film = rt.Film(W, H)
    st = film.render(scene_of(name), 1, max_depth=50, seed=SEED, variant=variant)
    pixels = film.download().reshape(N, 3)
    pixels.setflags(write=False)
    return pixels, int(st.rays)


@functools.lru_cache(maxsize=None)
def radiance_of(name, variant=0):
    """One sample along the render's camera rays from the render's streams, every output, computed once and shared."""
    o, d, tm, states = rays_of(name)
    out, st = scene_of(name).radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=variant, want=ALL, stats=True)
    return frozen(out), (int(st.rays), int(st.kernel_vgprs), int(st.scratch_bytes))


# ---- 1. the render, bit for bit ----
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_square_root_of_the_radiance_is_the_rendered_pixel_bit_for_bit(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    pixels, render_rays = render_of(name)
    out, (rays, vgprs, scratch) = radiance_of(name)
    path_rays = out["path_rays"]
    print(f"{name}: {vgprs} VGPRs, {scratch} B scratch; rays per path: " +
          ", ".join(f"{n}: {c}" for n, c in zip(*np.unique(path_rays, return_counts=True))))
    assert path_rays.min() >= 1 and path_rays.max() > 1, "some path is longer than one ray"
    if name.startswith("scene 9"):
        material = scene.intersect(o, d, times=tm, want=("material",))["material"]
        print(f"    {np.sum(material == 4)} first hits inside a medium")
        assert np.sum(material == 4) > 0, "some path enters a medium: the media draw from the ray's stream"
    assert np.array_equal(bits(np.sqrt(out["radiance"])), bits(pixels)), \
        f"{np.sum((bits(np.sqrt(out['radiance'])) != bits(pixels)).any(axis=-1))} of {N} pixels differ"
    assert int(path_rays.sum(dtype=np.uint64)) == render_rays, "the render traced the same rays"
    assert rays == render_rays, "stats.rays is the sum of path_rays"
    assert not np.array_equal(out["rng_state"], states), "the paths drew from their streams"


# ---- 2. closed forms ----
EMITTED = np.array((3.0, 2.5, 2.0))
SHELL_CENTRE = np.array((0.5, -0.25, 1.0))
MIRROR = np.array((0.8, 0.6, 0.2))


@functools.lru_cache(maxsize=None)
def shell_scene(world, mirror=False):
    """A light of radius 50 all around, a small sphere far outside it (a BVH world then has two leaves), and perhaps a perfect
    mirror inside it: the quad z = -5 seen from its front."""
    s = rt.Scene()
    items = [s.Sphere(SHELL_CENTRE, 50.0, s.DiffuseLight(EMITTED)), s.Sphere(SHELL_CENTRE + (500.0, 0.0, 0.0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]
    if mirror:
        items.append(s.Quad(SHELL_CENTRE + (-2.0, -2.0, -5.0), (4, 0, 0), (0, 4, 0), s.Metal(MIRROR, 0.0)))
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, (0.1, 0.1, 0.1))
    s.Commit()
    return s


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_inside_an_emissive_shell_every_ray_returns_the_emitted_colour(world, variant):
    gen = np.random.default_rng(5)
    start = gen.normal(size=(N, 3))
    start = SHELL_CENTRE + start / np.linalg.norm(start, axis=1, keepdims=True) * gen.uniform(0.0, 0.99, (N, 1))
    assert np.linalg.norm(start - SHELL_CENTRE, axis=1).max() < 1.0
    d = np.ascontiguousarray(gen.normal(size=(N, 3)) * gen.uniform(0.1, 10.0, (N, 1)))   # any direction, any length
    out = shell_scene(world).radiance(np.ascontiguousarray(start), d, samples=1, variant=variant, want=ALL)
    assert (out["radiance"] == EMITTED).all(), "0 + (1, 1, 1) * emitted: exact"
    assert (out["path_rays"] == 1).all()
    assert np.array_equal(out["rng_state"], host_states(SEED, 0, N)), "a light neither scatters nor draws"
    out = shell_scene(world).radiance(np.ascontiguousarray(start), d, samples=4, variant=variant, want=ALL)
    assert (out["radiance"] == EMITTED).all() and (out["path_rays"] == 4).all(), "0.25 * (4 x): exact"


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_a_perfect_mirror_returns_its_colour_times_the_emitted_colour(world, variant):
    gen = np.random.default_rng(6)
    start = gen.normal(size=(N, 3))
    start = SHELL_CENTRE + start / np.linalg.norm(start, axis=1, keepdims=True) * gen.uniform(0.0, 0.99, (N, 1))
    target = SHELL_CENTRE + np.stack([gen.uniform(-1.5, 1.5, N), gen.uniform(-1.5, 1.5, N), np.full(N, -5.0)], axis=-1)
    d = np.ascontiguousarray(target - start)   # towards the mirror's inside, at most ~40 degrees off its normal
    out = shell_scene(world, mirror=True).radiance(np.ascontiguousarray(start), d, samples=1, variant=variant, want=ALL)
    assert (out["radiance"] == MIRROR * EMITTED).all(), "0 + ((1, 1, 1) * albedo) * emitted: one product"
    assert (out["path_rays"] == 2).all()
    assert not np.array_equal(out["rng_state"], host_states(SEED, 0, N)), "Metal::Scatter draws its fuzz sample even at fuzz 0"


@functools.lru_cache(maxsize=None)
def closed_form_sphere():
    """The closed_form_sphere scene of tests/test_ray_query_gpu.py: a Lambertian (0.6, 0.4, 0.1) sphere in background (0.2, 0.3,
    0.9); no centre ray grazes it.  Returns (scene, origins, directions, background, albedo, which rays hit)."""
    bg_colour, centre, radius, colour = (0.2, 0.3, 0.9), (0.1, 0.05, -3.0), 0.8, (0.6, 0.4, 0.1)
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere(centre, radius, s.Lambertian(colour))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, bg_colour)
    s.Commit()
    o, d, _, bg = centre_rays(s, W, H)
    _, _, rel_disc = sphere_roots(o, d, centre, radius)
    assert not (np.abs(rel_disc) <= 1e-9).any(), "no centre ray of this set grazes the sphere"
    hits = rel_disc > 0
    assert 0.33 < hits.mean() < 0.35
    return s, o, d, bg, np.asarray(colour), hits


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_a_lambertian_sphere_in_a_bright_background(variant):
    """A convex body's scattered ray never returns to it: from max_depth 2 on a hitting ray is albedo * background after two rays."""
    s, o, d, bg, albedo, hits = closed_form_sphere()
    seeded = host_states(SEED, 0, N)
    for max_depth in (2, 3, 50):
        out = s.radiance(o, d, samples=1, max_depth=max_depth, variant=variant, want=ALL)
        assert (out["radiance"][hits] == albedo * bg).all(), "0 + ((1, 1, 1) * albedo) * background: one product"
        assert (out["radiance"][~hits] == bg).all()
        assert (out["path_rays"][hits] == 2).all() and (out["path_rays"][~hits] == 1).all()
        assert np.array_equal(out["rng_state"][~hits], seeded[~hits]), "a miss draws nothing"
        assert (out["rng_state"][hits] != seeded[hits]).any(axis=1).all(), "Lambertian::Scatter draws"
    out = s.radiance(o, d, samples=2, max_depth=2, variant=variant, want=ALL)
    assert (out["radiance"][hits] == albedo * bg).all() and (out["radiance"][~hits] == bg).all(), "0.5 * (x + x): exact"
    assert (out["path_rays"][hits] == 4).all() and (out["path_rays"][~hits] == 2).all()
    out = s.radiance(o, d, samples=1, max_depth=1, variant=variant, want=ALL)
    assert (out["radiance"][hits] == 0).all() and (out["radiance"][~hits] == bg).all(), "the one bounce is used up at the sphere"
    assert (out["path_rays"] == 1).all()
    out = s.radiance(o, d, samples=3, max_depth=0, variant=variant, want=ALL)
    assert (out["radiance"] == 0).all() and not np.signbit(out["radiance"]).any() and (out["path_rays"] == 0).all()
    assert np.array_equal(out["rng_state"], seeded), "nothing drawn: the state that goes out is the state that went in"
    mine = host_states(77, 1000, N)
    out = s.radiance(o, d, rng_state=mine, samples=3, max_depth=0, variant=variant, want=ALL)
    assert np.array_equal(out["rng_state"], mine) and (out["radiance"] == 0).all()


# ---- 3. streams ----
STREAM_SCENES = ["mixed bvh", "scene 9 list"]


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_library_seeding_equals_host_seeding(name):
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    for seed, first in ((SEED, 0), (7, 5), (SEED, (1 << 40) + 3)):
        seeded = scene.radiance(o, d, times=tm, seed=seed, first_sequence=first, want=ALL)
        handed = scene.radiance(o, d, times=tm, rng_state=host_states(seed, first, N), seed=123, first_sequence=9, want=ALL)
        assert same(seeded, handed), (seed, first)
    assert not same(seeded, radiance_of(name)[0], ("radiance",)), "another stream, another path"


def _raw_device_call(scene, dev_o, dev_d, dev_tm, count, samples, state_in, radiance, path_rays, state_out, first_sequence=0):
    """rt_scene_radiance_device on torch tensors of the caller's (any may be None where the interface allows NULL)."""
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    p = _lib.RadianceParams(count, samples, 50, 0.0, SEED, first_sequence, 0, 0, None)
    rays = _lib.RadianceRays(ptr(dev_o), ptr(dev_d), ptr(dev_tm), ptr(state_in))
    out = _lib.RadianceOut(ptr(radiance), ptr(path_rays), ptr(state_out))
    torch.cuda.synchronize()
    status = api.lib().rt_scene_radiance_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    assert status == 0, api.lib().rt_last_error().decode()


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_two_samples_are_two_calls_chained_through_the_state(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    first, _ = radiance_of(name)
    second = scene.radiance(o, d, times=tm, rng_state=np.ascontiguousarray(first["rng_state"]), samples=1, want=ALL)
    both = scene.radiance(o, d, times=tm, rng_state=states, samples=2, want=ALL)
    assert np.array_equal(bits(both["radiance"]), bits(0.5 * (first["radiance"] + second["radiance"])))
    assert np.array_equal(both["path_rays"], first["path_rays"] + second["path_rays"])
    assert np.array_equal(both["rng_state"], second["rng_state"])
    assert not np.array_equal(bits(first["radiance"]), bits(second["radiance"])), "the second sample is another path"
    # the same chain on the device with the state written back onto the array it was read from
    dev_o, dev_d, dev_tm = (torch.from_numpy(np.array(a)).cuda() for a in (o, d, tm))
    state = torch.from_numpy(states.view(np.int32).copy()).cuda()
    radiance = [torch.zeros((N, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
    path_rays = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(2)]
    for k in range(2):
        _raw_device_call(scene, dev_o, dev_d, dev_tm, N, 1, state, radiance[k], path_rays[k], state)
    assert np.array_equal(bits(radiance[0].cpu().numpy()), bits(first["radiance"])) and np.array_equal(bits(radiance[1].cpu().numpy()), bits(second["radiance"]))
    assert np.array_equal(state.cpu().numpy().view(np.uint32), both["rng_state"])
    assert np.array_equal((path_rays[0] + path_rays[1]).cpu().numpy().view(np.uint32), both["path_rays"])


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_a_split_batch_continues_the_streams(name):
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    whole = scene.radiance(o, d, times=tm, samples=2, want=ALL)
    split = 301
    head = scene.radiance(o[:split].copy(), d[:split].copy(), times=tm[:split].copy(), samples=2, want=ALL)
    tail = scene.radiance(o[split:].copy(), d[split:].copy(), times=tm[split:].copy(), samples=2, first_sequence=split, want=ALL)
    for key in ALL:
        assert np.array_equal(bits(np.concatenate([head[key], tail[key]])), bits(whole[key])), key
    restarted = scene.radiance(o[split:].copy(), d[split:].copy(), times=tm[split:].copy(), samples=2)   # without it: other streams
    assert not np.array_equal(bits(restarted["radiance"]), bits(whole["radiance"][split:]))


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_permuted_rays_with_their_states_give_permuted_results(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole, _ = radiance_of(name)
    order = np.random.default_rng(3).permutation(N)
    got = scene.radiance(np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), times=np.ascontiguousarray(tm[order]),
                         rng_state=np.ascontiguousarray(states[order]), want=ALL)
    for key in ALL:
        assert np.array_equal(bits(got[key]), bits(whole[key][order])), key


# ---- 4. plumbing ----
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_batch_edges_write_exactly_their_rays(count):
    guard_f, guard_i = 12345.678, 0x5A5A5A5A
    for name in ("mixed bvh", "mixed list"):
        scene = scene_of(name)
        o, d, tm, states = rays_of(name)
        whole, _ = radiance_of(name)
        dev_o, dev_d, dev_tm = (torch.from_numpy(np.array(a)).cuda() for a in (o, d, tm))   # longer than count: only count rays are read
        state = torch.from_numpy(states.view(np.int32).copy()).cuda()
        radiance = torch.full((N + 1, 3), guard_f, dtype=torch.float64, device="cuda")
        path_rays = torch.full((N + 1,), guard_i, dtype=torch.int32, device="cuda")
        state_out = torch.full((N + 1, 6), guard_i, dtype=torch.int32, device="cuda")
        _raw_device_call(scene, dev_o, dev_d, dev_tm, count, 1, state, radiance, path_rays, state_out)
        radiance, path_rays, state_out = radiance.cpu().numpy(), path_rays.cpu().numpy(), state_out.cpu().numpy()
        assert np.array_equal(bits(radiance[:count]), bits(whole["radiance"][:count])), name
        assert np.array_equal(path_rays[:count].view(np.uint32), whole["path_rays"][:count]), name
        assert np.array_equal(state_out[:count].view(np.uint32), whole["rng_state"][:count]), name
        assert (radiance[count:] == guard_f).all() and (path_rays[count:] == guard_i).all() and (state_out[count:] == guard_i).all(), \
            f"{name}: something behind ray {count - 1} was written"
        assert np.array_equal(state.cpu().numpy().view(np.uint32), states), "the states that came in were only read"


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_rays_without_a_direction_terminate_and_leave_their_neighbours_alone(name):
    """A zero or non-finite direction: at most samples * max_depth bounded searches, whatever comes back (include/rtow.h)."""
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole, _ = radiance_of(name)
    count = 64
    o, d, tm, states = (np.array(a[:count]) for a in (o, d, tm, states))
    odd = {0: (0.0, 0.0, 0.0), 9: (np.nan, 0.0, -1.0), 18: (np.inf, 0.0, -1.0), 27: (-np.inf, np.inf, np.nan), 36: (0.0, 0.0, 1e-320)}
    for k, direction in odd.items():
        d[k] = direction
    o[45] = (np.nan, 0.0, 0.0)
    tm[54] = np.nan
    out = scene.radiance(o, d, times=tm, rng_state=states, samples=2, max_depth=5, want=ALL)
    assert (out["path_rays"] <= 2 * 5).all() and (out["path_rays"] >= 2).all()
    good = np.ones(count, dtype=bool)
    good[list(odd) + [45, 54]] = False
    again = scene.radiance(o[good], d[good], times=tm[good], rng_state=states[good], samples=2, max_depth=5, want=ALL)
    for key in ALL:
        assert np.array_equal(bits(out[key][good]), bits(again[key])), key
    assert np.isfinite(out["radiance"][good]).all()


@pytest.mark.parametrize("name", ["mixed bvh", "scene 9 list"])
def test_each_output_alone_is_that_output_among_all(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole, (rays, _, _) = radiance_of(name)
    for key in ALL:
        alone, st = scene.radiance(o, d, times=tm, rng_state=states, want=(key,), stats=True)
        assert list(alone) == [key]
        assert np.array_equal(bits(alone[key]), bits(whole[key])), key
        assert st.rays == rays, "the searches are counted whether or not path_rays is asked for"
    assert same(scene.radiance(o, d, times=tm, rng_state=states, want=ALL), whole), "... and without statistics"


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_statistics_count_the_searches_and_leave_the_outputs_alone(name):
    """A call with statistics (two events and a counter word around the kernel) against the plain launch: the same outputs bit for
    bit.  100 rays are one full wave and a ragged one for the count's reduction over each wave."""
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    o, d = o[:100].copy(), d[:100].copy()
    plain = scene.radiance(o, d, time=time0, samples=2, variant=0, want=ALL)
    counted, st = scene.radiance(o, d, time=time0, samples=2, variant=0, want=ALL, stats=True)
    print(f"{name}: {st.rays} searches for 100 rays x 2 samples, {st.kernel_vgprs} VGPRs, {st.seconds * 1e3:.3f} ms")
    assert same(counted, plain)
    assert st.rays == plain["path_rays"].sum(dtype=np.uint64) and st.rays >= 200
    assert st.kernel_vgprs > 0 and st.seconds > 0


def test_torch_tensors_are_read_in_place_and_leave_films_alone():
    name = "scene 7 bvh"
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole, _ = radiance_of(name)
    film = rt.Film(W, H)
    before_stats = film.render(scene, 2, variant=0)
    before = film.download()
    dev_o, dev_d, dev_tm = (torch.from_numpy(np.array(a)).cuda() for a in (o, d, tm))
    for dev_states in (torch.from_numpy(np.array(states)).cuda(), torch.from_numpy(states.view(np.int32).copy()).cuda()):
        kept = [t.clone() for t in (dev_o, dev_d, dev_tm, dev_states)]
        out = scene.radiance(dev_o, dev_d, times=dev_tm, rng_state=dev_states, want=ALL)
        for key, a in out.items():
            assert isinstance(a, torch.Tensor) and a.device == dev_o.device
            got = a.cpu().numpy()
            assert np.array_equal(bits(got.view(np.uint32) if got.dtype == np.int32 else got), bits(whole[key])), key
        assert out["rng_state"].dtype == dev_states.dtype and out["path_rays"].dtype == torch.uint32
        for t, k in zip((dev_o, dev_d, dev_tm, dev_states), kept):
            assert np.array_equal(t.cpu().numpy(), k.cpu().numpy()), "the inputs are only read"
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # the current stream is the one the query runs on (and waits for)
        seeded = scene.radiance(dev_o, dev_d, time=0.0, samples=2)
    assert isinstance(seeded["radiance"], torch.Tensor)
    assert np.array_equal(bits(seeded["radiance"].cpu().numpy()), bits(scene.radiance(o, d, time=0.0, samples=2)["radiance"]))
    for bad in (dev_o.float(), dev_o.t().contiguous().t(), torch.from_numpy(np.array(o))):
        with pytest.raises(rt.RtowError):
            scene.radiance(bad, dev_d)
    for kw in (dict(rng_state=states), dict(rng_state=dev_states.long()), dict(rng_state=dev_states.t().contiguous().t()), dict(times=tm)):
        with pytest.raises(rt.RtowError):
            scene.radiance(dev_o, dev_d, **kw)
    with pytest.raises(rt.RtowError):
        scene.radiance(dev_o, d)   # a numpy array beside a tensor
    after_stats = film.render(scene, 2, variant=0)
    assert np.array_equal(bits(film.download()), bits(before)), "the same frame before and after the queries"
    assert (before_stats.rays, before_stats.samples, before_stats.kernel_kind, before_stats.lds_bytes) == \
        (after_stats.rays, after_stats.samples, after_stats.kernel_kind, after_stats.lds_bytes)


@pytest.mark.parametrize("scene_id, pixel, spp", [(7, (13, 9), 1), (8, (16, 12), 3)])
def test_rtow_radiance_at_prints_what_the_api_returns(scene_id, pixel, spp):
    i, j = pixel
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    run = subprocess.run([exe, "--scene", str(scene_id), "--width", str(W), "--height", str(H), "--variant", "strict", "--spp", str(spp),
                          "--radiance-at", f"{i},{j}"], check=True, cwd=ROOT, timeout=120, capture_output=True, text=True)
    lines = [line for line in run.stdout.splitlines() if line.startswith("radiance ")]
    assert len(lines) == 1 and run.stdout.count("\n") == 1, run.stdout
    words = lines[0].split()
    assert words[1] == f"{i},{j}:" and [words[k] for k in (2, 4, 8, 10)] == ["samples", "radiance", "rays", "seconds"], lines[0]
    scene = rt.builtin_scene(scene_id, 0, W, H)
    o, d, time0, _ = centre_rays(scene, W, H)
    k = j * W + i
    out = scene.radiance(o[k:k + 1].copy(), d[k:k + 1].copy(), time=time0, samples=spp, first_sequence=k, want=("radiance", "path_rays"))
    assert int(words[3]) == spp
    assert [float(x) for x in words[5:8]] == list(out["radiance"][0])
    assert int(words[9]) == out["path_rays"][0] and out["path_rays"][0] >= spp
    assert float(words[11]) > 0.0, "the kernel's time"


# ---- 5. strict against fast ----
def _share_that_differs(a, b):
    """The share of rows (rays, pixels) of which some channel differs by more than 1e-9 relative."""
    return float(np.mean((np.abs(a - b) > 1e-9 * np.maximum(np.abs(a), np.abs(b))).any(axis=-1)))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_strict_and_fast_differ_no_more_often_than_the_render_kernels_do(name):
    """A contracted comparison that falls the other way redraws the rest of a path, so some rays differ between the builds.  The
    yardstick is the render kernels on the same frame: the share of pixels of the 1-spp strict and fast frames that differ."""
    query = _share_that_differs(radiance_of(name, 0)[0]["radiance"], radiance_of(name, 1)[0]["radiance"])
    render = _share_that_differs(render_of(name, 0)[0], render_of(name, 1)[0])
    print(f"{name}: strict and fast differ by more than 1e-9 on {query * N:.0f} of {N} rays (radiance queries), "
          f"{render * N:.0f} of {N} pixels (render kernels)")
    assert query <= render + 8 / 768
