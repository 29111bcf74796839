"""The rehearsal keeps its samples (csrc/launch_plan.cpp plan_frame: probe_keeps, probe_ray_cap): the probe launch is the frame's
first probe_spp samples, the frame launch resumes from the streams and sums it saved; a rehearsed pixel that reaches the ray cap
stops there, saves nothing and is rendered from its first sample.  Every case is compared with its twin -- the same render with
RT_FLAG_NO_PIXEL_CLASSES | RT_FLAG_ROW_MAJOR_TILES, which plans no rehearsal at all: the frame bit for bit, the ray and sample
counts, and the streams the launch leaves behind (a second launch that continues them on both films gives equal frames again).
256 x 256 is the smallest frame that is rehearsed (1024 tiles, 65 536 pixels).  tests/test_rehearsal_plan.py has the plans."""
import numpy as np
import pytest
import torch

import raytracinginoneweekendincuda_amd as rt
from query_helpers import bits

pytestmark = pytest.mark.gpu

TWIN = rt.FLAG_NO_PIXEL_CLASSES | rt.FLAG_ROW_MAJOR_TILES
KEEP, ACCUMULATE = rt.FLAG_KEEP_RNG_STATE, rt.FLAG_ACCUMULATE
VARIANTS = [0, 1]   # the strict and the fast build


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def plans(scene, film, spp, variant, flags=0, adaptive=False, **kw):
    """The plan of the launch and of its twin; the twin must plan no rehearsal."""
    mine = scene.plan_launch(film.params(spp, variant=variant, flags=flags, **kw), num_cus=num_cus(), adaptive=adaptive)
    twin = scene.plan_launch(film.params(spp, variant=variant, flags=flags | TWIN, **kw), num_cus=num_cus(), adaptive=adaptive)
    assert (twin["probe_spp"], twin["probe_keeps"], twin["probe_ray_cap"]) == (0, 0, 0)
    return mine, twin


def render_pair(scene, w, h, spp, variant, film_kw=None, continue_with=3, **kw):
    """Render on a film and on its twin, compare frame, rays, samples and the continued streams.  Returns (film, twin film, plan)."""
    film_kw = film_kw or {}
    a, b = rt.Film(w, h, **film_kw), rt.Film(w, h, **film_kw)
    plan, _ = plans(scene, a, spp, variant, **kw)
    flags = kw.pop("flags", 0)
    st_a = a.render(scene, spp, variant=variant, flags=flags, **kw)
    st_b = b.render(scene, spp, variant=variant, flags=flags | TWIN, **kw)
    rows = rt.stripe_rows(h, a.stripe_rows, a.rank, a.world_size)
    assert (st_a.kernel_kind, st_a.pixels) == (st_b.kernel_kind, st_b.pixels)
    assert (st_a.rays, st_a.samples) == (st_b.rays, st_b.samples) and st_a.samples == st_a.pixels * spp
    assert np.array_equal(bits(a.download()[rows]), bits(b.download()[rows]))
    a.costs = a.probe_costs() if plan["pixel_classes"] else None   # of this launch: the continued one below rehearses nothing
    if continue_with:
        st_a = a.render(scene, continue_with, variant=variant, flags=flags | KEEP, **kw)
        st_b = b.render(scene, continue_with, variant=variant, flags=flags | KEEP | TWIN, **kw)
        assert (st_a.rays, st_a.samples) == (st_b.rays, st_b.samples)
        assert np.array_equal(bits(a.download()[rows]), bits(b.download()[rows]))
    return a, b, plan


# scene 11 as a list: the sphere-list kernel (kind 16).  (w, h, spp) -> probe_spp, classes, ray cap
SPHERE_LIST = [((256, 256, 64), (4, 1, 48)), ((256, 256, 400), (8, 1, 96)), ((256, 256, 32), (1, 0, 0)), ((255, 257, 64), (1, 0, 0))]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size,want", SPHERE_LIST)
def test_sphere_list(size, want, variant):
    """Classes with the cap at 48 and at 96 rays, a frame launch of 31 samples behind one rehearsed, and 65 535 pixels: ranked
    tiles without classes -- kept, no cap.  The glass sphere is in view: where there is a cap, pixels reach it."""
    w, h, spp = size
    scene = rt.builtin_scene(11, 1, w, h)
    film, _, plan = render_pair(scene, w, h, spp, variant, continue_with=0)
    assert plan["kernel_kind"] == 16 and plan["probe_keeps"] == 1
    assert (plan["probe_spp"], plan["pixel_classes"], plan["probe_ray_cap"]) == want
    if plan["probe_ray_cap"]:
        costs = film.costs
        capped = int(np.count_nonzero(costs >= plan["probe_ray_cap"]))
        print(f"{w} x {h} x {spp} variant {variant}: {capped} pixels stopped at {plan['probe_ray_cap']} rays, highest cost {costs.max()}")
        assert capped > 0 and costs.max() == plan["probe_ray_cap"]    # they stop at the cap, not behind it
    else:
        with pytest.raises(rt.RtowError):
            film.probe_costs()
    render_pair(scene, w, h, spp, variant)   # once more with the streams continued (fresh films)


@pytest.mark.parametrize("variant", VARIANTS)
def test_library_tree_world(variant):
    """Scene 0 as a BvhNode world: the library's tree (kind 64), classes with the longest chains one to a wave."""
    scene = rt.builtin_scene(0, 0, 256, 256)
    _, _, plan = render_pair(scene, 256, 256, 64, variant)
    assert (plan["kernel_kind"], plan["probe_spp"], plan["probe_keeps"], plan["pixel_classes"], plan["probe_ray_cap"]) == (64, 4, 1, 1, 120)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("waves", [4, 5])
def test_cornell_box(waves, variant):
    """Scene 7: the instanced list scan, on four waves per SIMD and on five, the build that parks the path state (and, in the
    rehearsal, its ray count) in LDS: 1120 pixels per compute unit are two generations on the lanes of four waves and one on those
    of five (560 x 512 on the 256 compute units of an MI355X)."""
    w, h = (256, 256) if waves == 4 else (560, 2 * num_cus())
    scene = rt.builtin_scene(7, 0, w, h)
    _, _, plan = render_pair(scene, w, h, 32, variant)
    assert (plan["kernel_kind"], plan["waves_per_simd"]) == (10, waves)
    assert (plan["rank_tiles"], plan["probe_spp"], plan["probe_keeps"], plan["probe_ray_cap"]) == (1, 1, 1, 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_final_scene(earth, variant):
    """Scene 9 with the committed earth bytes: the deep kernel (media draw random numbers inside the walk), ranking only."""
    scene = rt.builtin_scene(9, 0, 256, 256, earth=earth)
    _, _, plan = render_pair(scene, 256, 256, 32, variant)
    assert (plan["kernel_kind"], plan["rank_tiles"], plan["pixel_classes"], plan["probe_spp"], plan["probe_keeps"]) == (263, 1, 0, 1, 1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("max_depth", [0, 1])
def test_depth_limits(max_depth, variant):
    """No bounce at all (no ray is counted, every pixel black) and one: nobody reaches the cap, everything is kept."""
    scene = rt.builtin_scene(11, 1, 256, 256)
    film, _, plan = render_pair(scene, 256, 256, 64, variant, max_depth=max_depth)
    assert (plan["probe_keeps"], plan["probe_ray_cap"]) == (1, 48)
    assert film.costs.max() == (0 if max_depth == 0 else 4)


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_rank_of_three(variant):
    """Rank 1 of 3 with 8-row stripes of a 256 x 768 film owns 256 rows: 1024 tiles, 65 536 pixels -- rehearsed with classes."""
    w, h = 256, 768
    scene = rt.builtin_scene(11, 1, w, h)
    film, _, plan = render_pair(scene, w, h, 64, variant, film_kw=dict(stripe_rows=8, rank=1, world_size=3))
    assert (plan["probe_spp"], plan["pixel_classes"], plan["probe_keeps"], plan["probe_ray_cap"]) == (4, 1, 1, 48)
    rows = rt.stripe_rows(h, 8, 1, 3)
    costs = film.costs
    assert len(rows) == 256 and np.count_nonzero(costs[rows] >= 48) > 0
    others = np.setdiff1d(np.arange(h), rows)
    assert not costs[others].any()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("each", [32, 64])
def test_accumulated_launches(each, variant):
    """Two launches of 32 (one rehearsed sample, kept) and of 64 (four, classes, the cap) that add to the film's running sums equal
    one launch of twice as many, and the twin; the rehearsal of the second launch continues from those sums.  A plain launch on the
    same film afterwards is a plain launch."""
    w = h = 256
    scene = rt.builtin_scene(11, 1, w, h)
    film, twin = rt.Film(w, h), rt.Film(w, h)
    rays = [0, 0]
    for k in range(2):
        for n, (f, extra) in enumerate(((film, 0), (twin, TWIN))):
            rays[n] += f.render(scene, each, variant=variant, flags=ACCUMULATE | KEEP | extra).rays
    one = rt.Film(w, h)
    st_one = one.render(scene, 2 * each, variant=variant)
    assert rays[0] == rays[1] == st_one.rays
    assert np.array_equal(bits(film.download()), bits(twin.download()))
    assert np.array_equal(bits(film.download()), bits(one.download()))
    assert (film.sample_counts() == 2 * each).all()
    # a plain launch (re-seeded, not accumulated) after the accumulated frame, then one that continues its streams
    fresh = rt.Film(w, h)
    for flags in (0, KEEP):
        st_a = film.render(scene, each, variant=variant, flags=flags)
        st_b = fresh.render(scene, each, variant=variant, flags=flags | TWIN)
        assert st_a.rays == st_b.rays
        assert np.array_equal(bits(film.download()), bits(fresh.download()))


@pytest.mark.parametrize("variant", VARIANTS)
def test_adaptive_film_keeps_nothing(variant):
    """An adaptive film's rehearsal still only counts rays (probe_keeps 0; the cap holds for it too): frame, sample counts, rays and
    samples equal its twin's, and so does a second launch of the accumulated frame, which leaves the stopped pixels alone."""
    w = h = 256
    scene = rt.builtin_scene(11, 1, w, h)
    film, twin = rt.Film(w, h), rt.Film(w, h)
    for f in (film, twin):
        f.set_adaptive(8, 8, 0.05)
    plan, _ = plans(scene, film, 64, variant, flags=ACCUMULATE | KEEP, adaptive=True)
    assert (plan["probe_spp"], plan["pixel_classes"], plan["probe_keeps"], plan["probe_ray_cap"]) == (4, 1, 0, 48)
    for launch in range(2):
        st_a = film.render(scene, 64, variant=variant, flags=ACCUMULATE | KEEP)
        st_b = twin.render(scene, 64, variant=variant, flags=ACCUMULATE | KEEP | TWIN)
        assert (st_a.rays, st_a.samples) == (st_b.rays, st_b.samples)
        assert np.array_equal(film.sample_counts(), twin.sample_counts())
        assert np.array_equal(bits(film.download()), bits(twin.download()))
        if launch == 0:
            stopped = film.sample_counts() < 64
            assert stopped.any() and not stopped.all()
            before = film.sample_counts().copy()
    assert np.array_equal(film.sample_counts()[stopped], before[stopped])   # the marks held
    assert np.count_nonzero(film.probe_costs() >= 48) > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_films_in_flight(variant):
    """Two rehearsed frames on two streams at once, each with planes of its own: each equals its twin rendered alone."""
    w = h = 256
    jobs = [(11, 1, 64), (0, 0, 64)]
    scenes = [rt.builtin_scene(sid, world, w, h) for sid, world, _ in jobs]
    films = [rt.Film(w, h) for _ in jobs]
    for s, f, (_, _, spp) in zip(scenes, films, jobs):
        f.launch(s, f.params(spp, variant=variant))
    stats = [f.finish(s) for s, f in zip(scenes, films)]
    for s, f, st, (sid, _, spp) in zip(scenes, films, stats, jobs):
        twin = rt.Film(w, h)
        st_twin = twin.render(s, spp, variant=variant, flags=TWIN)
        assert (st.rays, st.samples) == (st_twin.rays, st_twin.samples), sid
        assert np.array_equal(bits(f.download()), bits(twin.download())), sid


def test_band_through_the_glass_sphere_equals_the_oracle(oracle):
    """Strict build, scene 11 at 256 x 256 x 64: eight rows through the glass sphere -- rows that hold pixels the cap stopped --
    bit for bit what the CPU oracle renders."""
    w = h = 256
    scene = rt.builtin_scene(11, 1, w, h)
    film = rt.Film(w, h)
    film.render(scene, 64, variant=0)
    stopped = film.probe_costs() >= 48
    r0 = int(np.argmax(stopped.reshape(h // 8, 8 * w).sum(axis=1))) * 8   # the band of eight rows that holds the most of them
    r1 = r0 + 8
    capped = int(np.count_nonzero(stopped[r0:r1]))
    want = oracle.render(11, 1, w, h, 64, rows=(r0, r1))
    got = film.download()
    exact = float(np.mean(np.all(bits(got[r0:r1]) == bits(want[r0:r1]), axis=-1)))
    print(f"rows {r0}..{r1 - 1}: {capped} pixels stopped at the cap, bit-exact {exact:.6f}, max |d| {np.abs(got[r0:r1] - want[r0:r1]).max():.3g}")
    assert capped > 0
    assert np.array_equal(bits(got[r0:r1]), bits(want[r0:r1]))
