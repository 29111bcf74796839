"""Adaptive sampling on the GPU (rt_film_set_adaptive): a pixel stops at the first check point where its noise is below the
threshold, and its value is then -- bit for bit -- what a plain render of that many samples gives for that pixel.

The checks: the values against the CPU oracle at every pixel's own count (4) and against the library's own fixed-spp path in
both builds through every instantiation (5), the counts against the rule applied to the oracle's frames (6), off is off (7),
progressive frames (8), the threshold's extremes (9), the executable (10).  test_adaptive_host.py holds the rule itself,
the prediction from the oracle (`predict_counts`) and the guard for the inputs used here."""
import os
import subprocess

import numpy as np
import pytest

import raytracinginoneweekendincuda_amd as rt
from query_helpers import bits
from test_adaptive_host import CAP, FLOOR, MIN, STEP, oracle_frames, predict_counts, rule_numpy
from test_custom_scenes_gpu import NESTINGS

pytestmark = pytest.mark.gpu

ADAPTIVE = 512   # rt_render_stats.kernel_kind
KEEP, ACC = rt.FLAG_KEEP_RNG_STATE, rt.FLAG_ACCUMULATE
TOL = 1e-5
CHECKS = list(range(MIN, CAP + 1, STEP))

# (scene, world kind, W, H, tau): min_samples 16, check_interval 16, cap 128, luminance floor 0.01.  On the oracle alone every stopping
# point is populated in every row and no pixel comes nearer to the threshold than 3e-5 relative.
TABLE = [(10, 1, 48, 32, 0.05), (11, 1, 48, 32, 0.05), (0, 0, 48, 32, 0.05), (7, 0, 32, 32, 0.25), (8, 0, 32, 32, 0.25), (3, 0, 32, 32, 0.05),
         (9, 0, 32, 32, 0.1)]
# what tests/test_parity_gpu.py asks of the strict build at fixed spp: (min bit-exact, min within 1e-5); the scenes without Perlin noise
# (device sin) or media (device log) are bit-exact
PARITY = {10: (1.0, 1.0), 11: (1.0, 1.0), 0: (1.0, 1.0), 7: (1.0, 1.0), 8: (0.98, 0.999), 3: (0.94, 0.999), 9: (0.98, 0.999)}

_FRAMES = {}


def frames_of(oracle, scene_id, world_kind, w, h):
    """the oracle's frames at 1 .. 128 spp (once per session)"""
    key = (scene_id, world_kind, w, h)
    if key not in _FRAMES:
        _FRAMES[key] = oracle_frames(oracle, scene_id, world_kind, w, h)
    return _FRAMES[key]


def adaptive_film(w, h, tau, min_samples=MIN, check_interval=STEP, **film_kw):
    film = rt.Film(w, h, **film_kw)
    film.set_adaptive(min_samples, check_interval, tau, FLOOR)
    return film


def adaptive_render(scene, w, h, cap, tau, **kw):
    film = adaptive_film(w, h, tau)
    st = film.render(scene, cap, **kw)
    return film.download(), film.sample_counts(), st


# ---- 4: values against the oracle ----
@pytest.mark.parametrize("scene_id,world_kind,w,h,tau,with_earth", [(*row, False) for row in TABLE] + [(*TABLE[-1], True)])
def test_values_equal_the_oracles_at_every_pixels_own_count(oracle, earth, scene_id, world_kind, w, h, tau, with_earth):
    e = earth if with_earth else None
    scene = rt.builtin_scene(scene_id, world_kind, w, h, earth=e)
    got, counts, st = adaptive_render(scene, w, h, CAP, tau, variant=0)
    values, pixels = np.unique(counts, return_counts=True)
    print(f"scene {scene_id}: counts {dict(zip(values.tolist(), pixels.tolist()))}, kernel kind {st.kernel_kind}")
    assert set(values.tolist()) <= set(CHECKS), values
    assert len(values) >= 4, "vacuous: fewer than four distinct stopping points"
    assert st.samples == int(counts.sum()) and st.pixels == w * h
    assert st.kernel_kind & ADAPTIVE
    want = np.zeros_like(got)
    for c in values.tolist():
        frame = oracle.render(scene_id, world_kind, w, h, c, earth=e) if (with_earth or (scene_id, world_kind, w, h) not in _FRAMES) \
            else _FRAMES[(scene_id, world_kind, w, h)][c]
        want[counts == c] = frame[counts == c]
    exact = np.mean(np.all(bits(got) == bits(want), axis=-1))
    within = np.mean(np.all(np.abs(got - want) <= TOL, axis=-1))
    print(f"scene {scene_id}: bit-exact {exact:.4f}, within {TOL:g}: {within:.4f}, max |d| {np.abs(got - want).max():.3g}")
    min_exact, min_within = PARITY[scene_id]
    assert within >= min_within and exact >= min_exact, (scene_id, exact, within)


# ---- 5: values against the fixed-spp path, both builds, every instantiation ----
def _builtin(scene_id, world_kind, w, h, earth=None):
    return lambda: rt.builtin_scene(scene_id, world_kind, w, h, earth=earth)


def _custom(name):
    def make():
        s = rt.Scene()
        NESTINGS[name](s, rt.Rng)
        return s
    return make


def instantiation_cases(earth):
    """(name, scene maker, W, H, cap, tau, render keywords, kernel kind without the adaptive bit, the general kernel's deep form
    -- one 768-thread workgroup per CU with the tables in more than 64 KB of LDS; told apart by that for kind 7 only)"""
    F = rt
    return [
        ("sphere list", _builtin(11, 1, 48, 32), 48, 32, 128, 0.05, {}, 16, False),
        ("sphere list, three spheres", _builtin(10, 1, 48, 32), 48, 32, 128, 0.05, {}, 16, False),
        ("sphere list, exact scan", _builtin(11, 1, 48, 32), 48, 32, 128, 0.05, dict(flags=F.FLAG_EXACT_SCAN), 16, False),
        ("sphere list, 8 pixels per wave", _builtin(11, 1, 48, 32), 48, 32, 128, 0.05, dict(pixels_per_wave=8), 16, False),
        ("sphere list, heavy and light pixels", _builtin(11, 1, 512, 256), 512, 256, 64, 0.05, dict(pixels_per_wave=0), 16, False),
        ("sphere list, one queue", _builtin(11, 1, 512, 256), 512, 256, 64, 0.05, dict(pixels_per_wave=0, flags=F.FLAG_NO_PIXEL_CLASSES), 16, False),
        ("list through the library's tree", _builtin(11, 1, 48, 32), 48, 32, 128, 0.05, dict(flags=F.FLAG_ACCELERATE_LISTS), 64, False),
        ("library tree", _builtin(0, 0, 48, 32), 48, 32, 128, 0.05, {}, 64, False),
        ("library tree, heavy and light pixels", _builtin(0, 0, 512, 256), 512, 256, 64, 0.05, dict(pixels_per_wave=0), 64, False),
        ("reference tree", _builtin(0, 0, 48, 32), 48, 32, 128, 0.05, dict(flags=F.FLAG_REFERENCE_TREE), 0, False),
        ("list scan, primitives (small BVH world)", _builtin(10, 0, 48, 32), 48, 32, 128, 0.05, {}, 8, False),
        ("list scan, primitives (list with moving spheres)", _builtin(0, 1, 48, 32), 48, 32, 128, 0.05, {}, 8, False),
        ("list scan, primitives, 16 pixels per wave", _builtin(10, 0, 48, 32), 48, 32, 128, 0.05, dict(pixels_per_wave=16), 8 + 128, False),
        ("list scan, instances", _builtin(7, 0, 32, 32), 32, 32, 128, 0.25, {}, 10, False),
        ("list scan, instances, list world", _builtin(7, 1, 32, 32), 32, 32, 128, 0.25, {}, 10, False),
        ("list scan, instances, 16 pixels per wave", _builtin(7, 0, 32, 32), 32, 32, 128, 0.25, dict(pixels_per_wave=16), 10 + 128, False),
        ("list scan, instances, the five-wave build's frame", _builtin(7, 0, 800, 800), 800, 800, 48, 0.25, {}, 10, False),
        ("BVH walk, instances", _builtin(7, 0, 32, 32), 32, 32, 128, 0.25, dict(flags=F.FLAG_ALWAYS_WALK), 2, False),
        ("BVH walk, media", _builtin(8, 0, 32, 32), 32, 32, 128, 0.25, {}, 6, False),
        ("BVH walk, general (forced)", _builtin(7, 0, 32, 32), 32, 32, 128, 0.25, dict(flags=F.FLAG_FORCE_GENERAL), 7, False),
        ("BVH walk, general (Perlin)", _builtin(3, 0, 32, 32), 32, 32, 128, 0.05, {}, 7, False),
        ("list, general (smoke)", _builtin(8, 1, 32, 32), 32, 32, 128, 0.25, {}, 15, False),
        ("list, general (Perlin)", _builtin(3, 1, 32, 32), 32, 32, 128, 0.05, {}, 15, False),
        ("BVH walk, general, deep", _builtin(9, 0, 32, 32, earth), 32, 32, 128, 0.1, dict(flags=F.FLAG_REFERENCE_TREE), 7, True),
        ("segmented walk", _builtin(9, 0, 32, 32, earth), 32, 32, 128, 0.1, {}, 7 + 256, False),
        ("segmented walk, heavy and light pixels", _builtin(9, 0, 512, 256, earth), 512, 256, 64, 0.1, dict(pixels_per_wave=0), 7 + 256, False),
        ("nested, BVH world", _custom("medium_in_medium"), 64, 32, 128, 0.1, {}, 7 + 32, False),
        ("nested, list world", _custom("list_of_lists_world"), 64, 32, 128, 0.1, {}, 15 + 32, False),
    ]


# every instantiation launch_one can reach with adaptive on: (kind, deep form of the general kernel)
ALL_KINDS = {(16, False), (0, False), (64, False), (8, False), (10, False), (8 + 128, False), (10 + 128, False), (15, False), (15 + 32, False),
             (2, False), (6, False), (7, False), (7, True), (7 + 256, False), (7 + 32, False)}


@pytest.mark.parametrize("variant", [0, 1])
def test_every_instantiation_equals_the_fixed_spp_path(earth, variant):
    """Adaptive frames against plain renders of the same scene at spp = each count, pixel for pixel, bit for bit, in both
    builds.  Kinds reached (rt_render_stats.kernel_kind without the adaptive bit): 16 sphere list (pixel-parallel, exact scan,
    grouped at 8 pixels per wave, with heavy / super lists and serving waves, and with one queue), 64 library tree (also with
    its lists, and for a list world), 0 reference tree, 8 and 10 list scans over primitives and instances, 136 and 138 the same
    with leaves dealt to lanes, 15 general list, 47 nested list, 2 BVH instances, 6 BVH media, 7 general shallow, 7 general
    deep (768 threads), 263 segmented (also with serving waves), 39 nested BVH: all fifteen.  The five-wave build of the
    instanced list scan (Traits::PARK) has no adaptive form by design: its frame is rendered by the four-wave build, which is
    asserted here."""
    reached, wrong = set(), []
    for name, make, w, h, cap, tau, kw, kind, big in instantiation_cases(earth):
        scene = make()
        got, counts, st = adaptive_render(scene, w, h, cap, tau, variant=variant, **kw)
        values, pixels = np.unique(counts, return_counts=True)
        print(f"{name}: kind {st.kernel_kind}, {st.kernel_vgprs} VGPRs, {st.lds_bytes} B LDS, counts {dict(zip(values.tolist(), pixels.tolist()))}")
        assert st.kernel_kind & ADAPTIVE, name
        deep = st.kernel_kind == 7 + ADAPTIVE and st.lds_bytes > 64 * 1024
        if (st.kernel_kind, deep) != (kind + ADAPTIVE, big):
            wrong.append((name, st.kernel_kind, st.lds_bytes))   # (reported at the end: the values are compared all the same)
        assert st.samples == int(counts.sum()), name
        assert set(values.tolist()) <= set(range(MIN, cap + 1, STEP)) and len(values) >= 2, (name, values)
        for c in values.tolist():
            want, pst = scene.render(w, h, c, variant=variant, **kw)
            assert pst.kernel_kind + ADAPTIVE == st.kernel_kind and pst.samples == w * h * c, (name, pst.kernel_kind)
            assert np.array_equal(bits(got)[counts == c], bits(want)[counts == c]), (name, c)
            if "five-wave" in name:
                assert pst.kernel_vgprs <= 96 < st.kernel_vgprs <= 128, (pst.kernel_vgprs, st.kernel_vgprs)
        reached.add((st.kernel_kind - ADAPTIVE, deep))
    assert not wrong, wrong
    assert reached == ALL_KINDS, (ALL_KINDS - reached, reached - ALL_KINDS)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("variant", [0, 1])
def test_striped_films_render_their_rows_of_the_adaptive_frame(world, variant):
    w, h, tau = 48, 32, 0.05
    for scene_id, world_kind in ((10, 1), (7, 0)):
        scene = rt.builtin_scene(scene_id, world_kind, w, h)
        t = 0.25 if scene_id == 7 else tau
        full, counts, st = adaptive_render(scene, w, h, CAP, t, variant=variant)
        samples = rays = 0
        for r in range(world):
            film = adaptive_film(w, h, t, stripe_rows=8, rank=r, world_size=world)
            pst = film.render(scene, CAP, variant=variant)
            rows = rt.stripe_rows(h, 8, r, world)
            others = [j for j in range(h) if j not in rows]
            part, pc = film.download(), film.sample_counts()
            assert np.array_equal(bits(part[rows]), bits(full[rows])) and np.array_equal(pc[rows], counts[rows])
            assert not pc[others].any()
            assert pst.samples == int(pc.sum()) and pst.kernel_kind & ADAPTIVE
            samples += pst.samples
            rays += pst.rays
        assert samples == st.samples and rays == st.rays


# ---- 6: the counts against the rule on the oracle ----
@pytest.mark.parametrize("scene_id,world_kind,w,h,tau", TABLE[:4])
def test_counts_equal_the_rule_applied_to_the_oracles_frames(oracle, scene_id, world_kind, w, h, tau):
    frames = frames_of(oracle, scene_id, world_kind, w, h)
    want, gap = predict_counts(frames, tau)
    scene = rt.builtin_scene(scene_id, world_kind, w, h)
    _, counts, st = adaptive_render(scene, w, h, CAP, tau, variant=0)
    decidable = gap > 1e-6
    left_out = int((~decidable).sum())
    differing = int((counts[decidable] != want[decidable]).sum())
    print(f"scene {scene_id}: {left_out} pixels left out (closest {gap.min():.3g}), {differing} counts differ; "
          f"predicted {dict(zip(*[x.tolist() for x in np.unique(want, return_counts=True)]))}")
    assert left_out <= 0.005 * w * h
    assert differing == 0


# ---- 2 (device part) and 7: parameters, off is off ----
def test_set_adaptive_validates_and_refuses_while_in_flight():
    scene = rt.builtin_scene(10, 1, 48, 32)
    film = rt.Film(48, 32)
    for bad in ((1, 16, 0.05, 0.01), (16, 0, 0.05, 0.01), (16, 16, -0.05, 0.01), (16, 16, float("nan"), 0.01), (16, 16, 0.05, 0.0),
                (16, 16, 0.05, -1.0)):
        with pytest.raises(rt.RtowError, match="status 1"):
            film.set_adaptive(*bad)
    film.set_adaptive(16, 16, 0.05)
    film.launch(scene, film.params(CAP, variant=0))
    with pytest.raises(rt.RtowError, match="status 5"):
        film.set_adaptive(None)
    st = film.finish(scene)
    assert st.kernel_kind & ADAPTIVE
    film.set_adaptive(None)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("scene_id,world_kind", [(10, 1), (7, 0), (9, 0)])
def test_off_is_off(scene_id, world_kind, variant):
    w, h, spp = 48, 32, 6
    scene = rt.builtin_scene(scene_id, world_kind, w, h)
    plain = rt.Film(w, h)
    a = plain.render(scene, spp, variant=variant)
    fa = plain.download().copy()
    assert np.array_equal(plain.sample_counts(), np.full((h, w), spp, dtype=np.uint32))
    b = plain.render(scene, spp, variant=variant, flags=KEEP)
    fb = plain.download().copy()
    film = adaptive_film(w, h, 0.1)
    film.render(scene, 64, variant=variant)
    assert len(np.unique(film.sample_counts())) >= 2
    film.set_adaptive(None)
    c = film.render(scene, spp, variant=variant)
    fc = film.download().copy()
    assert np.array_equal(film.sample_counts(), np.full((h, w), spp, dtype=np.uint32))
    d = film.render(scene, spp, variant=variant, flags=KEEP)
    fd = film.download().copy()
    assert np.array_equal(bits(fa), bits(fc)) and np.array_equal(bits(fb), bits(fd))
    for x, y in ((a, c), (b, d)):
        assert (x.rays, x.samples, x.kernel_kind, x.kernel_vgprs) == (y.rays, y.samples, y.kernel_kind, y.kernel_vgprs)
        assert x.samples == w * h * spp and not (x.kernel_kind & ADAPTIVE)
    # accumulated frames count their launches
    acc = rt.Film(w, h)
    acc.render(scene, 2, variant=variant, flags=ACC)
    acc.render(scene, 3, variant=variant, flags=ACC | KEEP)
    assert np.array_equal(acc.sample_counts(), np.full((h, w), 5, dtype=np.uint32))


# ---- 8: progressive ----
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("scene_id,world_kind,tau", [(10, 1, 0.05), (8, 0, 0.25)])
def test_accumulated_launches_equal_one_launch(scene_id, world_kind, tau, variant):
    w, h = (48, 32) if scene_id == 10 else (32, 32)
    scene = rt.builtin_scene(scene_id, world_kind, w, h)
    one, one_counts, one_st = adaptive_render(scene, w, h, 128, tau, variant=variant)
    film = adaptive_film(w, h, tau)
    samples = rays = 0
    for k in range(4):
        st = film.render(scene, 32, variant=variant, flags=ACC | (KEEP if k else 0))
        samples += st.samples
        rays += st.rays
        assert st.kernel_kind & ADAPTIVE
    four, four_counts = film.download().copy(), film.sample_counts().copy()
    assert np.array_equal(bits(four), bits(one)) and np.array_equal(four_counts, one_counts)
    assert samples == one_st.samples == int(one_counts.sum()) and rays == one_st.rays
    assert len(np.unique(one_counts)) >= 4
    # a fifth launch: only the pixels that stood at the cap unconverged go on -- the frame is the one of a single launch of 160
    st5 = film.render(scene, 32, variant=variant, flags=ACC | KEEP)
    five, five_counts = film.download().copy(), film.sample_counts().copy()
    more = five_counts.astype(np.int64) - four_counts
    assert np.all(more >= 0) and np.all(more[four_counts < 128] == 0) and more.any()
    assert st5.samples == int(more.sum())
    assert np.array_equal(bits(five)[more == 0], bits(four)[more == 0])
    longer, longer_counts, _ = adaptive_render(scene, w, h, 160, tau, variant=variant)
    assert np.array_equal(bits(five), bits(longer)) and np.array_equal(five_counts, longer_counts)
    assert np.all(longer_counts[four_counts < 128] == four_counts[four_counts < 128])
    # other parameters, or none, in the middle of the accumulated frame
    film.set_adaptive(MIN, STEP, tau * 2, FLOOR)
    with pytest.raises(rt.RtowError, match="status 5"):
        film.render(scene, 32, variant=variant, flags=ACC | KEEP)
    film.set_adaptive(None)
    with pytest.raises(rt.RtowError, match="status 5"):
        film.render(scene, 32, variant=variant, flags=ACC | KEEP)
    film.set_adaptive(MIN, STEP, tau, FLOOR)          # set back: the frame goes on
    film.render(scene, 0, variant=variant, flags=ACC | KEEP)
    assert np.array_equal(bits(film.download()), bits(five)) and np.array_equal(film.sample_counts(), five_counts)
    film.set_adaptive(MIN, STEP, tau * 2, FLOOR)      # a re-seeding launch begins a frame with whatever is set
    st = film.render(scene, 128, variant=variant, flags=ACC)
    other, other_counts, other_st = adaptive_render(scene, w, h, 128, tau * 2, variant=variant)
    assert np.array_equal(bits(film.download()), bits(other)) and np.array_equal(film.sample_counts(), other_counts) and st.samples == other_st.samples


# ---- 9: threshold extremes ----
def test_threshold_extremes(oracle):
    w, h = 48, 32
    scene = rt.builtin_scene(10, 1, w, h)
    frames = frames_of(oracle, 10, 1, w, h)
    got, counts, st = adaptive_render(scene, w, h, CAP, 1e6, variant=0)
    assert np.all(counts == MIN) and st.samples == MIN * w * h
    assert np.array_equal(bits(got), bits(frames[MIN]))
    # tau = 1e-3 stops a pixel only where its samples so far are all the same colour: one ray into the sky in each of the first 16
    # (the oracle's frames at 1 .. 16 spp are constant there, up to the rounding of c added n times), 533 pixels; every other pixel
    # runs to the cap.  395 of the 533 are sky in all 128 samples; the other 138 lie on silhouettes and meet a sphere later -- the
    # rule's known weakness (csrc/adaptive_rule.h), which min_samples guards, and they stop all the same.
    sky = np.all(np.abs(frames[1:MIN + 1] - frames[1:2]) <= 1e-12, axis=(0, 3))
    always_sky = np.all(np.abs(frames[1:] - frames[1:2]) <= 1e-12, axis=(0, 3))
    want, gap = predict_counts(frames, 1e-3)
    assert int(sky.sum()) == 533 and int(always_sky.sum()) == 395 and np.all(sky[always_sky])
    assert np.array_equal(want == MIN, sky) and np.all(want[~sky] == CAP) and gap.min() > 0.5
    got, counts, st = adaptive_render(scene, w, h, CAP, 1e-3, variant=0)
    assert np.array_equal(counts == MIN, sky) and np.all(counts[~sky] == CAP)
    assert st.samples == 533 * MIN + 1003 * CAP
    assert np.array_equal(bits(got)[sky], bits(frames[MIN])[sky]) and np.array_equal(bits(got)[~sky], bits(frames[CAP])[~sky])


# ---- 10: the executable ----
def test_rtow_noise_and_samples_map(tmp_path):
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    w, h = 48, 32
    base = ["--scene", "10", "--width", str(w), "--height", str(h), "--variant", "strict"]
    a, m, b, c = tmp_path / "a.ppm", tmp_path / "m.pgm", tmp_path / "b.ppm", tmp_path / "c.ppm"
    r = subprocess.run([exe, *base, "--spp", "128", "--noise", "0.05", "--min-spp", "16", "--check-every", "16", "--samples-map", str(m),
                        "--output", str(a)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    scene = rt.builtin_scene(10, 0, w, h)
    frame, counts, st = adaptive_render(scene, w, h, 128, 0.05, variant=0, pixels_per_wave=0)
    rt.write_ppm(b, frame)
    assert a.read_bytes() == b.read_bytes()
    head = f"P5\n{w} {h}\n65535\n".encode()
    raw = m.read_bytes()
    assert raw.startswith(head) and len(raw) == len(head) + 2 * w * h
    assert np.array_equal(np.frombuffer(raw[len(head):], dtype=">u2").reshape(h, w), counts[::-1])
    assert len(np.unique(counts)) >= 4
    assert f"{st.samples / (w * h):.2f} samples per pixel on average" in r.stderr
    # without --noise: the plain frame, and not a word about adaptive sampling
    r = subprocess.run([exe, *base, "--spp", "3", "--output", str(a)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    plain, _ = scene.render(w, h, 3, variant=0)
    rt.write_ppm(c, plain)
    assert a.read_bytes() == c.read_bytes()
    assert "adaptive" not in r.stderr and "Rendering a 48x32 image with 3 samples per pixel in 8x8 blocks." in r.stderr
    for bad in (["--samples-map", str(m)], ["--min-spp", "8"], ["--check-every", "4"], ["--noise", "-1"], ["--noise", "nan"], ["--noise", "abc"],
                ["--noise", "0.05x"], ["--noise", "inf"]):
        r = subprocess.run([exe, *base, *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--noise" in r.stderr, (bad, r.returncode, r.stderr)


def test_scene_render_takes_adaptive_and_returns_the_counts():
    w, h = 48, 32
    scene = rt.builtin_scene(10, 1, w, h)
    want, counts, st = adaptive_render(scene, w, h, CAP, 0.05, variant=0)
    for adaptive in ((MIN, STEP, 0.05), dict(min_samples=MIN, check_interval=STEP, noise_threshold=0.05, luminance_floor=FLOOR)):
        got, gst = scene.render(w, h, CAP, variant=0, adaptive=adaptive)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(gst.sample_counts, counts)
        assert gst.samples == st.samples == int(counts.sum()) and gst.kernel_kind == st.kernel_kind
    plain, pst = scene.render(w, h, 4, variant=0)
    assert not hasattr(pst, "sample_counts") and pst.samples == w * h * 4


@pytest.mark.parametrize("variant", [0, 1])
def test_no_build_fuses_the_rule(variant):
    """The rule as the adaptive kernels of each build compile it (rt_adaptive_rule_on_device), against the numpy restatement
    on sums placed within a few ulps of the threshold: a build that contracted q + y * y or q * N - s * s into a fused
    multiply-add (plain -ffp-contract=fast does, whatever the header's pragma says) rounds once where the rule rounds twice,
    and differs in q's last bit or in the decision on some of these."""
    rng = np.random.default_rng(5)
    for min_samples, check_interval, tau, floor in ((16, 16, 0.05, 0.01), (2, 1, 0.25, 0.01), (32, 32, 1e-3, 0.5)):
        k = 40000
        n = min_samples + check_interval * rng.integers(0, 12, k)
        N = n.astype(np.float64)
        mean = rng.random((k, 3)) * np.array([0.7, 1.0, 1.3])
        sums = mean * N[:, None]
        sample = rng.random((k, 3)) * 1.7
        s = (sums[:, 0] + sums[:, 1]) + sums[:, 2]
        y = (sample[:, 0] + sample[:, 1]) + sample[:, 2]
        m = np.maximum(s, floor * N)
        rhs = ((tau * tau) * (N - 1.0)) * (m * m)
        f = np.where(rng.random(k) < 0.6, 1.0 + rng.integers(-4, 5, k) * 2.0 ** -52, np.exp(rng.normal(0.0, 1.0, k)))
        q_after = (rhs * f + s * s) / N            # lhs lands around rhs
        q_before = q_after - y * y
        want_q = q_before + y * y
        want = rule_numpy(n, sums[:, 0], sums[:, 1], sums[:, 2], want_q, min_samples, check_interval, tau, floor)
        got_q, got = rt.adaptive_rule_on_device(n, np.column_stack([sums, q_before]), sample, min_samples, check_interval, tau, floor,
                                                variant=variant)
        assert 0.1 < want.mean() < 0.9
        assert np.array_equal(bits(got_q), bits(want_q)), int(np.sum(bits(got_q) != bits(want_q)))
        assert np.array_equal(got, want), int(np.sum(got != want))


def test_a_plain_launch_ends_an_accumulated_adaptive_frame():
    """set_adaptive(None), a launch without ACCUMULATE (it overwrites every pixel, the stopped ones too), the same parameters again:
    ACCUMULATE | KEEP_RNG_STATE then begins a frame on the continued streams instead of continuing over the overwritten pixels."""
    w, h, tau = 48, 32, 0.05
    scene = rt.builtin_scene(10, 1, w, h)
    film = adaptive_film(w, h, tau)
    film.render(scene, 64, variant=0, flags=ACC)
    assert (film.sample_counts() == MIN).any()
    film.set_adaptive(None)
    film.render(scene, 4, variant=0)
    film.set_adaptive(MIN, STEP, tau, FLOOR)
    st = film.render(scene, 64, variant=0, flags=ACC | KEEP)
    other = rt.Film(w, h)
    other.render(scene, 4, variant=0)
    other.set_adaptive(MIN, STEP, tau, FLOOR)
    ost = other.render(scene, 64, variant=0, flags=KEEP)
    assert np.array_equal(bits(film.download()), bits(other.download())) and np.array_equal(film.sample_counts(), other.sample_counts())
    assert st.samples == ost.samples == int(film.sample_counts().sum())
