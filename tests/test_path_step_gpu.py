"""Path steps (rt_scene_path_step, Scene.path_step): one bounce of RayColor for caller-supplied rays.  The keystone is the radiance
query, which existing tests pin to the render bit for bit: a host loop that steps the live rays, folds acc = acc + thr * emitted
and thr = thr * attenuation in numpy float64 and keeps the scattered rays is rt_scene_radiance -- its radiance, its ray counts and
its final streams -- bit for bit in the strict build.  Beside it the step against the ray query, one restatement of Lambertian
scatter that does not go through the library's shading, closed forms that are exact in both builds, the stream rules, the
plumbing (batch edges with guards, outputs left out, statistics, degenerate rays), the torch path with aliased arrays, and the
executable.  Every ray set is at most 32 x 24 rays."""
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
from query_helpers import bits, centre_rays
from test_radiance_gpu import SCENES, camera_rays, closed_form_sphere, host_states, shell_scene
from test_radiance_gpu import EMITTED, MIRROR, SHELL_CENTRE

pytestmark = pytest.mark.gpu

W, H = 32, 24
N = W * H
SEED = 1984
ALL = tuple(_lib.STEP_OUTPUTS)
MISS, ENDS, SCATTERED = 0, 1, 2

# the radiance tests' scenes and scene 12, whose triangle meshes sit under instances
STEP_SCENES = dict(SCENES, **{"scene 12 bvh": lambda: rt.builtin_scene(12, 0, W, H)})


def same(got, want, keys=ALL):
    return all(np.array_equal(bits(got[k]), bits(want[k])) for k in keys)


def frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return STEP_SCENES[name]()


@functools.lru_cache(maxsize=None)
def rays_of(name):
    """The camera rays of the scene's 1-spp render with their streams, computed once and shared (nobody writes to them)."""
    arrays = camera_rays(scene_of(name))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def step_of(name, variant=0):
    """The first step along the render's camera rays from the render's streams, every output, computed once and shared."""
    o, d, tm, states = rays_of(name)
    return frozen(scene_of(name).path_step(o, d, times=tm, rng_state=states, variant=variant, want=ALL))


# ---- 1. the fold is the radiance ----
def fold(scene, o, d, tm, states, max_depth, seen, variant=0):
    """One sample of RayColor by steps, as include/rtow.h states the fold: numpy float64, one operation a line, nothing fused.
    Returns (acc (n, 3), steps per ray (n,), the streams after the paths (n, 6)); the statuses and material kinds met go to `seen`."""
    n = len(o)
    acc, thr = np.zeros((n, 3)), np.ones((n, 3))
    steps, final = np.zeros(n, dtype=np.uint32), np.array(states)
    live = np.arange(n)
    o, d, tm, states = (np.array(a) for a in (o, d, tm, states))
    for _ in range(max_depth):
        if live.size == 0:
            break
        out = scene.path_step(o, d, times=tm, rng_state=states, variant=variant,
                              want=("status", "emitted", "attenuation", "origin", "direction", "time", "material", "rng_state"))
        status = out["status"]
        seen["status"].update(np.unique(status).tolist())
        seen["material"].update(np.unique(out["material"]).tolist())
        steps[live] += 1
        final[live] = out["rng_state"]
        ends, goes_on = status != SCATTERED, status == SCATTERED
        product = thr[live[ends]] * out["emitted"][ends]
        acc[live[ends]] = acc[live[ends]] + product
        thr[live[goes_on]] = thr[live[goes_on]] * out["attenuation"][goes_on]
        live = live[goes_on]
        o, d, tm, states = (np.ascontiguousarray(out[k][goes_on]) for k in ("origin", "direction", "time", "rng_state"))
    return acc, steps, final


SEEN = {"status": set(), "material": set()}   # over every fold of this module


@functools.lru_cache(maxsize=None)
def fold_of(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    want = scene.radiance(o, d, times=tm, rng_state=states, samples=1, max_depth=50, variant=0, want=("radiance", "path_rays", "rng_state"))
    return fold(scene, o, d, tm, states, 50, SEEN), want


@pytest.mark.parametrize("name", sorted(STEP_SCENES))
def test_the_fold_of_steps_is_the_radiance_bit_for_bit(name):
    (acc, steps, final), want = fold_of(name)
    print(f"{name}: steps per ray: " + ", ".join(f"{n}: {c}" for n, c in zip(*np.unique(steps, return_counts=True))))
    assert steps.max() > 1, "some path is longer than one ray"
    assert np.array_equal(bits(acc), bits(want["radiance"])), \
        f"{np.sum((bits(acc) != bits(want['radiance'])).any(axis=-1))} of {N} rays differ"
    assert np.array_equal(steps, want["path_rays"]), "a step a world search"
    assert np.array_equal(final, want["rng_state"]), "the streams end where the radiance query leaves them"


def test_three_samples_of_four_bounces_restart_and_cut_as_the_radiance_query_does():
    """The smallest case where the depth cut and the sample restart both happen: each sample restarts from the first ray with the
    stream where the previous sample left it, and the mean is (1 / samples) * (((0 + L_1) + L_2) + L_3)."""
    name, samples, max_depth = "mixed list", 3, 4
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    want = scene.radiance(o, d, times=tm, rng_state=states, samples=samples, max_depth=max_depth, variant=0, want=("radiance", "path_rays", "rng_state"))
    total, rays = np.zeros((N, 3)), np.zeros(N, dtype=np.uint32)
    cut = 0
    for _ in range(samples):
        acc, steps, states = fold(scene, o, d, tm, states, max_depth, SEEN)
        total = total + acc
        rays += steps
        cut += int(np.sum(steps == max_depth))
    mean = (1 / np.float64(samples)) * total
    assert cut > 0, "some path is cut at max_depth"
    assert np.array_equal(bits(mean), bits(want["radiance"]))
    assert np.array_equal(rays, want["path_rays"])
    assert np.array_equal(states, want["rng_state"])


def test_the_folds_saw_every_status_and_every_material_kind():
    for name in sorted(STEP_SCENES):
        fold_of(name)
    print(f"statuses {sorted(SEEN['status'])}, material kinds {sorted(SEEN['material'])}")
    assert SEEN["status"] == {MISS, ENDS, SCATTERED}
    assert SEEN["material"] == {0, 1, 2, 3, 4, 255}, "Lambertian, metal, dielectric, diffuse light, isotropic, and none for a miss"


# ---- 2. a step agrees with the ray query ----
HIT_RECORD = ("t", "normal", "front_face", "material")


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list", "scene 7 bvh", "scene 12 bvh"])
def test_the_hit_record_of_a_step_is_the_ray_querys(name):
    """Worlds without media: the search draws nothing, so the ray query needs no stream to find the same hit."""
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    step = step_of(name)
    query = scene.intersect(o, d, times=tm, want=HIT_RECORD)
    for key in HIT_RECORD:
        assert np.array_equal(bits(step[key]), bits(query[key])), key
    assert np.array_equal(step["status"] == MISS, np.isinf(step["t"])) and (step["t"] > 0).all()
    assert (step["status"] != MISS).any()


@pytest.mark.parametrize("name", ["scene 9 bvh", "scene 9 list"])
def test_with_media_a_seeded_step_finds_what_the_seeded_ray_query_finds(name):
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    for seed, first in ((SEED, 0), (7, 5)):
        step = scene.path_step(o, d, times=tm, seed=seed, first_sequence=first, want=("status",) + HIT_RECORD)
        query = scene.intersect(o, d, times=tm, seed=seed, first_sequence=first, want=HIT_RECORD)
        for key in HIT_RECORD:
            assert np.array_equal(bits(step[key]), bits(query[key])), (key, seed, first)
        assert np.array_equal(step["status"] == MISS, np.isinf(step["t"]))
    assert np.sum(step["material"] == 4) > 0, "some ray ends inside a medium: the media draw from the ray's stream"


# ---- 3. Lambertian scatter restated on the host ----
def test_a_lambertian_scatter_restated_with_the_hosts_generator():
    """Not through the library's shading: random_in_unit_sphere from rt.Rng(seed, k) in shade's order of draws (three uniforms a
    try, 2 * (a, b, c) - 1, until its squared length is below 1), the direction n + rs, the origin ray(t), the solid colour."""
    s, o, d, bg, albedo, hits = closed_form_sphere()
    first = 11
    query = s.intersect(o, d, want=("t", "normal"))
    out = s.path_step(o, d, time=0.25, seed=SEED, first_sequence=first, variant=0, want=ALL)
    assert np.array_equal(out["status"] == SCATTERED, hits) and np.array_equal(out["status"] == MISS, ~hits)
    want_o, want_d, want_state = np.array(o), np.array(d), np.zeros((N, 6), dtype=np.uint32)
    for k in range(N):
        rng = rt.Rng(SEED, k + first)
        if hits[k]:
            while True:
                a, b, c = np.float64(rng.uniform()), np.float64(rng.uniform()), np.float64(rng.uniform())
                rs = 2.0 * np.array([a, b, c]) - np.array([1.0, 1.0, 1.0])
                if (rs[0] * rs[0] + rs[1] * rs[1]) + rs[2] * rs[2] < 1.0:
                    break
            want_d[k] = query["normal"][k] + rs
            assert np.abs(want_d[k]).max() >= 1e-8   # (else Lambertian::Scatter takes the normal)
            want_o[k] = o[k] + query["t"][k] * d[k]
        want_state[k] = rng.state()
    assert np.array_equal(bits(out["direction"]), bits(want_d))
    assert np.array_equal(bits(out["origin"]), bits(want_o))
    assert (out["time"] == 0.25).all()
    assert (out["attenuation"][hits] == albedo).all() and (out["attenuation"][~hits] == 0).all()
    assert (out["emitted"][hits] == 0).all() and (out["emitted"][~hits] == bg).all()
    assert not np.signbit(out["emitted"]).any() and not np.signbit(out["attenuation"]).any()
    assert np.array_equal(out["rng_state"], want_state)
    assert (out["material"][hits] == 0).all() and (out["material"][~hits] == 255).all()


# ---- 4. closed forms, exact in both builds ----
def _starts(gen):
    """Points within a unit of the shell's centre on a grid of 1/64: differences and squares of such coordinates are exact."""
    return SHELL_CENTRE + gen.integers(-36, 37, size=(N, 3)) / 64.0


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_inside_an_emissive_shell_every_path_ends_with_the_emitted_colour(world, variant):
    gen = np.random.default_rng(5)
    start = np.ascontiguousarray(_starts(gen))
    d = np.ascontiguousarray(gen.normal(size=(N, 3)) * gen.uniform(0.1, 10.0, (N, 1)))   # any direction, any length
    tm = np.ascontiguousarray(gen.uniform(0.0, 1.0, N))
    out = shell_scene(world).path_step(start, d, times=tm, variant=variant, want=ALL)
    assert (out["status"] == ENDS).all()
    assert (out["emitted"] == EMITTED).all(), "0 + (1, 1, 1) * emitted: exact"
    assert (out["attenuation"] == 0).all() and not np.signbit(out["attenuation"]).any()
    assert np.array_equal(bits(out["origin"]), bits(start)) and np.array_equal(bits(out["direction"]), bits(d)) and np.array_equal(bits(out["time"]), bits(tm))
    assert (out["material"] == 3).all() and (out["front_face"] == 0).all() and np.isfinite(out["t"]).all()
    assert np.array_equal(out["rng_state"], host_states(SEED, 0, N)), "a light neither scatters nor draws"


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_a_perfect_mirror_scatters_its_albedo_along_the_reflection(world, variant):
    """Rays on the 1/64 grid towards the mirror z = centre - 5 (normal (0, 0, 1)): d . d is a sum of exact squares, so unit(d) is
    one square root, one division and a product per component whether or not the build contracts, and the reflection about an axis
    is exact."""
    gen = np.random.default_rng(6)
    start = np.ascontiguousarray(_starts(gen))
    target = SHELL_CENTRE + np.concatenate([gen.integers(-96, 97, size=(N, 2)) / 64.0, np.full((N, 1), -5.0)], axis=1)
    d = np.ascontiguousarray(target - start)
    out = shell_scene(world, mirror=True).path_step(start, d, variant=variant, want=ALL)
    assert (out["status"] == SCATTERED).all() and (out["material"] == 1).all() and (out["front_face"] == 1).all()
    assert (out["attenuation"] == MIRROR).all() and (out["emitted"] == 0).all()
    n = np.array([0.0, 0.0, 1.0])
    assert (out["normal"] == n).all()
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    ud = (1 / length)[:, None] * d
    cos = (ud[:, 0] * n[0] + ud[:, 1] * n[1]) + ud[:, 2] * n[2]
    reflected = ud - (2.0 * cos)[:, None] * n
    assert (out["direction"] == reflected).all(), "reflect(unit(d), n) + 0 * sample"
    assert np.abs(out["origin"][:, 2] - (SHELL_CENTRE[2] - 5.0)).max() < 1e-12, "the scattered ray starts on the mirror"
    assert not np.array_equal(out["rng_state"], host_states(SEED, 0, N)), "Metal::Scatter draws its fuzz sample even at fuzz 0"


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_a_miss_returns_the_background_and_the_ray_and_the_stream_as_they_came(variant):
    s, o, d, bg, _, hits = closed_form_sphere()
    miss = ~hits
    o, d = np.ascontiguousarray(o[miss]), np.ascontiguousarray(d[miss])
    tm = np.linspace(-1.0, 2.0, len(o))
    mine = host_states(77, 1000, len(o))
    out = s.path_step(o, d, times=tm, rng_state=mine, variant=variant, want=ALL)
    assert (out["status"] == MISS).all() and (out["emitted"] == bg).all() and (out["attenuation"] == 0).all()
    assert np.array_equal(bits(out["origin"]), bits(o)) and np.array_equal(bits(out["direction"]), bits(d)) and np.array_equal(bits(out["time"]), bits(tm))
    assert np.isposinf(out["t"]).all() and (out["normal"] == 0).all() and (out["front_face"] == 0).all() and (out["material"] == 255).all()
    assert np.array_equal(out["rng_state"], mine), "a miss draws nothing"


# ---- 5. streams and plumbing ----
STREAM_SCENES = ["mixed bvh", "scene 9 list"]


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_library_seeding_equals_host_seeding(name):
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    for seed, first in ((SEED, 0), (7, 5), (SEED, (1 << 40) + 3)):
        seeded = scene.path_step(o, d, times=tm, seed=seed, first_sequence=first, want=ALL)
        handed = scene.path_step(o, d, times=tm, rng_state=host_states(seed, first, N), seed=123, first_sequence=9, want=ALL)
        assert same(seeded, handed), (seed, first)
    assert not same(seeded, step_of(name), ("direction",)), "another stream, another scatter"


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_a_split_batch_continues_the_streams(name):
    scene = scene_of(name)
    o, d, tm, _ = rays_of(name)
    whole = scene.path_step(o, d, times=tm, want=ALL)
    split = 301
    head = scene.path_step(o[:split].copy(), d[:split].copy(), times=tm[:split].copy(), want=ALL)
    tail = scene.path_step(o[split:].copy(), d[split:].copy(), times=tm[split:].copy(), first_sequence=split, want=ALL)
    for key in ALL:
        assert np.array_equal(bits(np.concatenate([head[key], tail[key]])), bits(whole[key])), key
    restarted = scene.path_step(o[split:].copy(), d[split:].copy(), times=tm[split:].copy(), want=ALL)   # without it: other streams
    assert not np.array_equal(bits(restarted["direction"]), bits(whole["direction"][split:]))


@pytest.mark.parametrize("name", STREAM_SCENES)
def test_permuted_rays_with_their_states_give_permuted_results(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole = step_of(name)
    order = np.random.default_rng(3).permutation(N)
    got = scene.path_step(np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), times=np.ascontiguousarray(tm[order]),
                          rng_state=np.ascontiguousarray(states[order]), want=ALL)
    for key in ALL:
        assert np.array_equal(bits(got[key]), bits(whole[key][order])), key


GUARDS = {"float64": 12345.678, "uint8": 0x5A, "uint32": 0x5A5A5A5A}
TORCH_TYPES = {"float64": torch.float64, "uint8": torch.uint8, "uint32": torch.int32}


def _guarded_outputs(rows):
    return {name: torch.full((rows,) + tail, GUARDS[dtype], dtype=TORCH_TYPES[dtype], device="cuda") for name, (dtype, tail) in _lib.STEP_OUTPUTS.items()}


def _raw_device_call(scene, count, dev_o, dev_d, dev_tm, state_in, outs, first_sequence=0, stream=None):
    """rt_scene_path_step_device on torch tensors of the caller's; `outs`: name -> tensor for the outputs wanted."""
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    p = _lib.PathStepParams(count, 0.0, SEED, first_sequence, 0, 0, stream)
    rays = _lib.PathStepRays(ptr(dev_o), ptr(dev_d), ptr(dev_tm), ptr(state_in))
    out = _lib.PathStepOut(**{name: ptr(t) for name, t in outs.items()})
    torch.cuda.synchronize()
    status = api.lib().rt_scene_path_step_device(scene._p, C.byref(p), C.byref(rays), C.byref(out), None)
    assert status == 0, api.lib().rt_last_error().decode()


def _host(name, tensor):
    a = tensor.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_batch_edges_write_exactly_their_rays(count):
    for name in ("mixed bvh", "mixed list"):
        scene = scene_of(name)
        o, d, tm, states = rays_of(name)
        whole = step_of(name)
        dev_o, dev_d, dev_tm = (torch.from_numpy(np.array(a)).cuda() for a in (o, d, tm))   # longer than count: only count rays are read
        state = torch.from_numpy(states.view(np.int32).copy()).cuda()
        outs = _guarded_outputs(N + 1)
        _raw_device_call(scene, count, dev_o, dev_d, dev_tm, state, outs)
        for key, (dtype, _) in _lib.STEP_OUTPUTS.items():
            got = _host(key, outs[key])
            assert np.array_equal(bits(got[:count]), bits(whole[key][:count])), (name, key)
            guard = np.array(GUARDS[dtype]).astype(got.dtype)
            assert (got[count:] == guard).all(), f"{name}: {key}: something behind ray {count - 1} was written"
        assert np.array_equal(state.cpu().numpy().view(np.uint32), states), "the states that came in were only read"


@pytest.mark.parametrize("name", ["mixed bvh", "scene 9 list"])
def test_each_output_alone_is_that_output_among_all(name):
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole = step_of(name)
    scattered = int(np.sum(whole["status"] == SCATTERED))
    for key in ALL:
        alone, st = scene.path_step(o, d, times=tm, rng_state=states, want=(key,), stats=True)
        assert list(alone) == [key]
        assert np.array_equal(bits(alone[key]), bits(whole[key])), key
        assert st.rays == N and st.scattered == scattered, "the scattered rays are counted whether or not status is asked for"


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_statistics_count_the_scattered_rays_and_leave_the_outputs_alone(name):
    """A call with statistics (two events and a counter word around the kernel) against the plain launch: the same outputs bit for
    bit.  100 rays are one full wave and a ragged one for the count's ballot."""
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    o, d = o[:100].copy(), d[:100].copy()
    plain = scene.path_step(o, d, time=time0, variant=0, want=ALL)
    counted, st = scene.path_step(o, d, time=time0, variant=0, want=ALL, stats=True)
    print(f"{name}: {st.scattered} of {st.rays} rays scattered, {st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch, {st.seconds * 1e3:.3f} ms")
    assert same(counted, plain)
    assert st.rays == 100 and st.scattered == np.sum(plain["status"] == SCATTERED) and 0 < st.scattered
    assert st.kernel_vgprs > 0 and st.seconds > 0


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_rays_without_a_direction_terminate_and_leave_their_neighbours_alone(name):
    """A zero or non-finite direction: one bounded search, whatever comes back (include/rtow.h)."""
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    count = 64
    o, d, tm, states = (np.array(a[:count]) for a in (o, d, tm, states))
    odd = {0: (0.0, 0.0, 0.0), 9: (np.nan, 0.0, -1.0), 18: (np.inf, 0.0, -1.0), 27: (-np.inf, np.inf, np.nan), 36: (0.0, 0.0, 1e-320)}
    for k, direction in odd.items():
        d[k] = direction
    o[45] = (np.nan, 0.0, 0.0)
    tm[54] = np.nan
    out = scene.path_step(o, d, times=tm, rng_state=states, want=ALL)
    assert (out["status"] <= SCATTERED).all()
    good = np.ones(count, dtype=bool)
    good[list(odd) + [45, 54]] = False
    whole = step_of(name)
    for key in ALL:
        assert np.array_equal(bits(out[key][good]), bits(whole[key][:count][good])), key


# ---- 6. torch, in place ----
def test_torch_tensors_are_read_in_place_may_alias_and_leave_films_alone():
    name = "scene 7 bvh"
    scene = scene_of(name)
    o, d, tm, states = rays_of(name)
    whole = step_of(name)
    film = rt.Film(W, H)
    before_stats = film.render(scene, 2, variant=0)
    before = film.download()
    dev_o, dev_d, dev_tm = (torch.from_numpy(np.array(a)).cuda() for a in (o, d, tm))
    for dev_states in (torch.from_numpy(np.array(states)).cuda(), torch.from_numpy(states.view(np.int32).copy()).cuda()):
        kept = [t.clone() for t in (dev_o, dev_d, dev_tm, dev_states)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):   # the current stream is the one the step runs on (and waits for)
            out = scene.path_step(dev_o, dev_d, times=dev_tm, rng_state=dev_states, want=ALL)
        for key, a in out.items():
            assert isinstance(a, torch.Tensor) and a.device == dev_o.device
            assert np.array_equal(bits(_host(key, a)), bits(whole[key])), key
        assert out["rng_state"].dtype == dev_states.dtype and out["status"].dtype == torch.uint8
        for t, k in zip((dev_o, dev_d, dev_tm, dev_states), kept):
            assert np.array_equal(t.cpu().numpy(), k.cpu().numpy()), "the inputs are only read"
    # the outputs on top of the inputs of the same meaning: every lane reads its ray and its six words before it writes
    al_o, al_d, al_tm = dev_o.clone(), dev_d.clone(), dev_tm.clone()
    al_state = torch.from_numpy(states.view(np.int32).copy()).cuda()
    outs = {k: v for k, v in _guarded_outputs(N).items() if k not in ("origin", "direction", "time", "rng_state")}
    outs.update(origin=al_o, direction=al_d, time=al_tm, rng_state=al_state)
    _raw_device_call(scene, N, al_o, al_d, al_tm, al_state, outs)
    for key in ALL:
        assert np.array_equal(bits(_host(key, outs[key])), bits(whole[key])), key
    for bad in (dev_o.float(), dev_o.t().contiguous().t(), torch.from_numpy(np.array(o))):
        with pytest.raises(rt.RtowError):
            scene.path_step(bad, dev_d)
    for kw in (dict(rng_state=states), dict(rng_state=dev_states.long()), dict(times=tm)):
        with pytest.raises(rt.RtowError):
            scene.path_step(dev_o, dev_d, **kw)
    after_stats = film.render(scene, 2, variant=0)
    assert np.array_equal(bits(film.download()), bits(before)), "the same frame before and after the steps"
    assert (before_stats.rays, before_stats.samples, before_stats.kernel_kind, before_stats.lds_bytes) == \
        (after_stats.rays, after_stats.samples, after_stats.kernel_kind, after_stats.lds_bytes)


# ---- 7. the executable ----
def _rtow(scene_id, spp, option, pixel):
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    run = subprocess.run([exe, "--scene", str(scene_id), "--width", str(W), "--height", str(H), "--variant", "strict", "--spp", str(spp),
                          option, f"{pixel[0]},{pixel[1]}"], check=True, cwd=ROOT, timeout=120, capture_output=True, text=True)
    return run.stdout.splitlines()


@pytest.mark.parametrize("scene_id, pixel, spp", [(7, (13, 9), 1), (8, (16, 12), 3)])
def test_rtow_trace_at_ends_with_the_line_of_radiance_at(scene_id, pixel, spp):
    """The last line of --trace-at against the line of --radiance-at, up to the last field: `seconds` is the time of the kernels
    of that run, a measurement that no two runs share."""
    i, j = pixel
    trace = _rtow(scene_id, spp, "--trace-at", pixel)
    radiance = _rtow(scene_id, spp, "--radiance-at", pixel)
    assert len(radiance) == 1 and radiance[0].startswith(f"radiance {i},{j}: ")
    for line in trace[:-1]:
        words = line.split()
        assert [words[k] for k in (0, 1, 3, 5, 7, 9, 11, 15)] == ["vertex:", "sample", "depth", "status", "t", "material", "emitted", "attenuation"], line
        assert len(words) == 19
    got, got_seconds = trace[-1].rsplit(" seconds ", 1)
    want, want_seconds = radiance[0].rsplit(" seconds ", 1)
    assert got == want
    assert float(got_seconds) > 0.0 and float(want_seconds) > 0.0
    scene = rt.builtin_scene(scene_id, 0, W, H)
    o, d, time0, _ = centre_rays(scene, W, H)
    k = j * W + i
    out = scene.radiance(o[k:k + 1].copy(), d[k:k + 1].copy(), time=time0, samples=spp, first_sequence=k, want=("radiance", "path_rays"))
    assert len(trace) - 1 == out["path_rays"][0] and out["path_rays"][0] >= spp
    samples = [int(line.split()[2]) for line in trace[:-1]]
    assert sorted(set(samples)) == list(range(spp)) and samples == sorted(samples)
    statuses = [int(line.split()[6]) for line in trace[:-1]]
    depths = [int(line.split()[4]) for line in trace[:-1]]
    for a in range(len(trace) - 2):   # a scattered vertex is followed by the next depth of its sample, any other by depth 0 of the next
        assert (depths[a + 1], samples[a + 1]) == ((depths[a] + 1, samples[a]) if statuses[a] == SCATTERED and depths[a] + 1 < 50 else (0, samples[a] + 1))
