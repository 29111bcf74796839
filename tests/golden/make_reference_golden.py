#!/usr/bin/env python3
"""Generates tests/golden/reference_hits.npz: rays off the camera and what the reference's own classes answer for them.

Run by hand where the reference checkout is present, after `make -C oracle ref` (oracle/_ref/libref_world.so is the reference's
header-only classes compiled for the host, oracle/ref_world.cpp).  The file holds only data -- ray inputs, the outputs of
world->Hit, of one RayColor iteration and of whole paths for them, the frames of ref_render, bounding boxes -- and the GPU tests
(tests/test_reference_gpu.py) read it and nothing else of the reference.  tests/reference_worlds.py has the three worlds, the
layout of the file (Fixture) and its packing.

Per world 512 rays per set, from numpy.random.default_rng; every set is asserted here to do what it is for:

  free      origins uniform in the world's bounding box enlarged by a half, directions uniform on the sphere, scaled by 1e-3, 1 or 1e3
  inside    origins inside the glass sphere, inside each box and inside each medium's boundary (checked from the shapes'
            definitions); nearly half of them with a tmax short enough that some stop before the container's wall
  axis      directions with one or two components exactly 0.0 or -0.0: from random origins, from origins lying exactly on a coordinate
            of a leaf's bounding box with the zero on that axis (0 * inf in Aabb::Hit), and rays parallel or nearly parallel to each
            quad's plane (the 1e-8 rule of Quad::Hit)
  windows   free and inside rays again with (tmin, tmax) drawn around the reference's own T of the default window: tmax just below T,
            tmax just above T, tmin just above T, tmin = 0
  times     the movers' interval ends, its middle and values outside it on both sides (rays aimed at the movers where the world has
            some; free and inside rays again elsewhere)

Ray k of a hit set draws from curand_init(1984, k, 0), as Scene.intersect seeds it.  The step set is the free rays and then the
inside rays through RayColor's window with the committed `streams`; `radiance` is the fold of such steps along the whole path of the
inside rays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import reference_scene as R   # noqa: E402
import reference_worlds as RW   # noqa: E402

N = 512
OUT = os.path.join(ROOT, "tests", "golden", "reference_hits.npz")
INF = float("inf")
TIMES = np.array([-1.0, -0.25, 0.0, 0.5, 1.0, 1.25, 2.5])   # the movers' interval is 0 .. 1
NEAR = 2.0 ** -30                                           # "just" below or above T, relative


def grid(a, step):
    return np.rint(np.asarray(a, dtype=np.float64) / step) * step


def unit_directions(rng, n):
    """Uniform on the sphere, on a grid of 2^-10, never zero."""
    v = rng.normal(size=(n, 3))
    v = grid(v / np.linalg.norm(v, axis=-1, keepdims=True), 2.0 ** -10)
    assert np.all(np.any(v != 0, axis=-1))
    return v


def origin_step(box):
    """The power-of-two grid on which a world's origins fit 16-bit integers."""
    return 2.0 ** np.ceil(np.log2(np.abs(box).max() * 1.75 / 32000.0))


def seeded_streams(n, seed=RW.SEED, first=0):
    return np.array([R.RefRng(seed, first + k).state() for k in range(n)], dtype=np.uint32)


def draws_between(before, after, most=4096):
    """How many XORWOW steps lead from each state to the other (asserted to exist): the fixture keeps the count, not the words."""
    draws = np.full(len(before), -1, dtype=np.int64)
    cur = before.copy()
    for k in range(most + 1):
        same = np.all(cur == after, axis=-1) & (draws < 0)
        draws[same] = k
        if np.all(draws >= 0):
            break
        cur = RW.xorwow_advance(cur, np.ones(len(cur), dtype=np.int64))
    assert np.all(draws >= 0)
    assert np.array_equal(RW.xorwow_advance(before, draws), after)
    return draws


def sphere_uv(n):
    with np.errstate(invalid="ignore"):
        theta, phi = np.arccos(-n[:, 1]), np.arctan2(-n[:, 2], n[:, 0]) + np.pi
    return np.stack([phi / (2.0 * np.pi), theta / np.pi], axis=-1)


def hit_record(scene, o, d, time, tmin, tmax):
    """ref_hit of a set with the streams Scene.intersect gives its rays, as the fixture's record (RW.HIT_FIELDS)."""
    got = scene.hit(o, d, time, tmin, tmax, seeded_streams(len(o)))
    hit = got["hit"] != 0
    medium = hit & (got["material_handle"] == 0)
    assert np.all(got["material"][medium] == 4)
    outward = np.where((got["front_face"] != 0)[:, None], got["normal"], -got["normal"])
    on_sphere = hit & ~medium & (np.abs(sphere_uv(outward) - got["uv"]).max(axis=-1) < 1e-9)
    shape = np.where(~hit, 255, np.where(medium, 2, np.where(on_sphere, 0, 1))).astype(np.uint8)
    return {"hit": got["hit"], "t": got["t"], "normal": got["normal"], "uv": got["uv"], "front_face": got["front_face"],
            "material": got["material"], "shape": shape}


def make_sets(name, rng, ref, leaf_boxes, world_box):
    """The ray sets of a world: {set: dict(o, d (the base), factor, time, tmin, tmax)}; the windows come from ``ref``, the tree world."""
    step = origin_step(world_box)
    lo, hi = world_box[0::2], world_box[1::2]
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    default = dict(tmin=np.full(N, 0.001), tmax=np.full(N, INF))
    sets = {}

    # free
    sets["free"] = dict(o=grid(centre + 1.5 * half * rng.uniform(-1, 1, (N, 3)), step), d=unit_directions(rng, N), factor=rng.integers(0, 3, N),
                        time=grid(rng.random(N), 2.0 ** -8), **default)

    # inside
    boxes = RW.containers(name)
    share = [N // len(boxes) + (k < N % len(boxes)) for k in range(len(boxes))]
    o, d, tmax = [], [], []
    for (label, kind, params), n in zip(boxes, share):
        assert n >= 64, label
        p = grid(RW.sample_inside(rng, kind, params, n), 2.0 ** -12)
        assert np.all(RW.inside(p, kind, params)), label
        size = 2.0 * params[1] if kind == "sphere" else float(np.min(np.asarray(params[1]) - np.asarray(params[0])))
        dd = unit_directions(rng, n)
        short = rng.random(n) < 0.45
        o.append(p)
        d.append(dd)
        tmax.append(np.where(short, grid(size * rng.random(n), 2.0 ** -12), INF))
    factor = rng.integers(0, 3, N)
    tmax = np.concatenate(tmax)
    sets["inside"] = dict(o=np.concatenate(o), d=np.concatenate(d), factor=factor, time=grid(rng.random(N), 2.0 ** -8), tmin=np.full(N, 0.001),
                          tmax=np.where(np.isinf(tmax), INF, tmax / RW.FACTORS[factor]))   # (the length of d is about its factor)

    # axis
    zero = np.array([0.0, -0.0])
    n_a, n_b = 192, 192
    n_c = N - n_a - n_b
    d_a = unit_directions(rng, n_a)
    d_a[np.abs(d_a) < 2.0 ** -6] = 2.0 ** -6              # the zeros of this set are put there on purpose
    for k in range(n_a):
        axes = rng.choice(3, size=1 + k % 2, replace=False)
        d_a[k, axes] = rng.choice(zero, size=len(axes))
    o_a = grid(centre + half * rng.uniform(-1, 1, (n_a, 3)), step)
    which = rng.integers(0, len(leaf_boxes), n_b)           # on a coordinate of a leaf's box, the zero on that axis
    o_b, d_b = np.zeros((n_b, 3)), unit_directions(rng, n_b)
    d_b[np.abs(d_b) < 2.0 ** -6] = 2.0 ** -6
    for k in range(n_b):
        b = leaf_boxes[which[k]]
        blo, bhi = b[0::2], b[1::2]
        axis = k % 3
        span = np.minimum(bhi - blo, 8.0)                   # (the ground sphere's box is 200 wide: stay near its top)
        p = grid(bhi - span * rng.random(3), 2.0 ** -10)
        away = grid(bhi + 0.5 * rng.random(3), 2.0 ** -10)
        p = np.where(rng.random(3) < 0.4, away, p)          # some start outside the box on the other axes
        p[axis] = (blo, bhi)[(k // 3) % 2][axis]            # exactly, as the box holds it
        d_b[k, axis] = zero[(k // 6) % 2]
        if k % 4 == 0:                                      # and towards the box on the others
            d_b[k] = np.where(np.arange(3) == axis, d_b[k], grid(0.5 * (blo + bhi) - p, 2.0 ** -10))
        o_b[k] = p
    o_c, d_c = np.zeros((n_c, 3)), np.zeros((n_c, 3))       # in or nearly in a quad's plane
    planes = RW.quads(name)
    for k in range(n_c):
        q, u, v = (np.asarray(x, dtype=np.float64) for x in planes[k % len(planes)])
        normal = np.cross(u, v)
        normal /= np.linalg.norm(normal)
        a, b = rng.uniform(-1, 1, 2)
        tilt = (0.0, 0.5e-8, -0.5e-8, 2e-8, -2e-8, 1e-3)[(k // len(planes)) % 6]
        along = a * u + b * v
        d_c[k] = along / np.linalg.norm(along) + tilt * normal
        height = (0.0, 1e-9, -1e-9, 1e-4)[(k // (6 * len(planes))) % 4]
        o_c[k] = q + rng.random() * u + rng.random() * v - 0.5 * d_c[k] + height * normal
    o_axis, d_axis = np.concatenate([o_a, o_b, o_c]), np.concatenate([d_a, d_b, d_c])
    zeros = np.sum(d_axis[:n_a + n_b] == 0, axis=-1)
    assert np.all((zeros >= 1) & (zeros <= 2)) and np.any(np.signbit(d_axis) & (d_axis == 0)) and np.any(~np.signbit(d_axis) & (d_axis == 0))
    on_box = [o_b[k, k % 3] == leaf_boxes[which[k]][2 * (k % 3) + (k // 3) % 2] and d_b[k, k % 3] == 0 for k in range(n_b)]
    assert all(on_box), "0 * inf is met: the origin lies on the box's coordinate of the axis whose direction component is zero"
    sets["axis"] = dict(o=o_axis, d=d_axis, factor=np.concatenate([rng.integers(0, 3, n_a + n_b), np.ones(n_c, dtype=np.int64)]),
                        time=grid(rng.random(N), 2.0 ** -8), **default)

    # windows: around the reference's own T of the default window (the streams are those of this set's rays)
    def full(s):
        return s["o"], s["d"] * RW.FACTORS[s["factor"]][:, None], s["time"]

    both = {k: np.concatenate([sets["free"][k], sets["inside"][k]]) for k in ("o", "d", "factor", "time")}
    first = ref.hit(*full(both), 0.001, INF, seeded_streams(2 * N))
    ends_in_medium = (first["hit"] != 0) & (first["material_handle"] == 0)
    order = np.concatenate([np.flatnonzero(ends_in_medium)[:N // 2], np.flatnonzero((first["hit"] != 0) & ~ends_in_medium),
                            np.flatnonzero(first["hit"] == 0)])
    take = np.sort(np.concatenate([order[order < N][:N // 2], order[order >= N][:N // 2]]))
    if len(take) < N:
        take = np.sort(np.concatenate([take, np.setdiff1d(order, take)[:N - len(take)]]))
    chosen = {k: both[k][take] for k in both}
    base = ref.hit(*full(chosen), 0.001, INF, seeded_streams(N))
    T = np.where(base["hit"] != 0, base["t"], 1.0)
    mode = np.arange(N) % 4
    sets["windows"] = dict(chosen, again=take, tmin=np.where(mode == 2, T * (1 + NEAR), np.where(mode == 3, 0.0, 0.001)),
                           tmax=np.where(mode == 0, T * (1 - NEAR), np.where(mode == 1, T * (1 + NEAR), INF)))
    if RW.MEDIA[name]:
        in_medium = (base["hit"] != 0) & (base["material_handle"] == 0)
        assert in_medium.sum() >= 128, in_medium.sum()

    # times
    pick = rng.integers(0, len(TIMES), N)
    if name == "mixed":
        movers = [((-0.6, 0.8, -1.4), (-0.6, 1.1, -1.4), 0.25), ((1.5, 0.7, -0.8), (1.2, 0.7, -0.8), 0.2)]   # query_helpers.mixed_world
        o, d = np.zeros((N, 3)), np.zeros((N, 3))
        for k in range(N):
            c0, c1, radius = (np.asarray(x, dtype=np.float64) for x in movers[k % 2])
            when = TIMES[pick[k]] if (k // 2) % 2 else TIMES[rng.integers(0, len(TIMES))]   # half aim where the mover is at another time
            target = c0 + when * (c1 - c0) + 0.9 * radius * rng.uniform(-1, 1, 3)
            below = unit_directions(rng, 1)[0]
            below[1] = -abs(below[1])                       # from below: what passes the mover goes on to the sky
            o[k] = grid(target + 1.5 * below, 2.0 ** -10)
            d[k] = grid(target - o[k], 2.0 ** -10)
        sets["times"] = dict(o=o, d=d, factor=rng.integers(0, 3, N), time=TIMES[pick], **default)
    else:
        again = np.concatenate([np.arange(3 * N // 4), N + np.arange(N // 4)])
        sets["times"] = dict({k: both[k][again] for k in ("o", "d", "factor")}, again=again, time=TIMES[pick], **default)
    assert all(np.any(sets["times"]["time"] == t) for t in TIMES)
    return sets


def fold(scene, o, d, time, streams, depth=50):
    """acc += thr * emitted where a path ends, thr *= attenuation where it scatters, one operation at a time (include/rtow.h
    rt_scene_path_step), over ``depth`` steps.  Returns (radiance, exact): exact where no step of the path met a medium or a noise
    texture."""
    n = len(o)
    acc, thr, exact = np.zeros((n, 3)), np.ones((n, 3)), np.ones(n, dtype=bool)
    live = np.arange(n)
    o, d, time, streams = o.copy(), d.copy(), time.copy(), streams.copy()
    for _ in range(depth):
        if len(live) == 0:
            break
        s = scene.step(o, d, time, streams)
        exact[live] &= s["flags"] == 0
        ended = s["status"] != 2
        acc[live[ended]] = acc[live[ended]] + thr[live[ended]] * s["emitted"][ended]
        thr[live[~ended]] = thr[live[~ended]] * s["attenuation"][~ended]
        live = live[~ended]
        o, d, time, streams = s["origin"][~ended], s["direction"][~ended], s["time"][~ended], s["rng_state"][~ended]
    return acc, exact


def generate(verbose=False):
    """Every array of the fixture, as a dict."""
    def say(*a):
        if verbose:
            print(*a)

    def put(key, kind, a):   # the list world's array only where it is not the tree world's (Fixture.of)
        if kind == 0 or not np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(out[key + "0"]).view(np.uint8)):
            out[f"{key}{kind}"] = a

    import raytracinginoneweekendincuda_amd as rt
    out = {"streams": np.array([RW.xorwow_advance(seeded_streams(1, RW.SEED + 1, k), [k % 5])[0] for k in range(2 * N)], dtype=np.uint32)}
    seen_status, seen_kinds, seen_faces, metal_absorbs = set(), set(), set(), 0
    for w, name in enumerate(RW.WORLDS):
        rng = np.random.default_rng(1984 + w)
        refs = {}
        for kind in RW.KINDS:
            refs[kind] = RW.Recorder(R.RefScene())
            RW.build(name, refs[kind], R.RefRng, kind)
            put(f"{name}/boxes", kind, np.array([refs[kind].scene.BoundingBox(h) for h in refs[kind].hittables]))
            put(f"{name}/frame", kind, refs[kind].scene.render(RW.W, RW.H, RW.SPP, RW.SEED))
        product = RW.build(name, rt.Scene(), rt.Rng, 0)
        leaf_boxes = product.dump_leaves()[1]
        world_box = out[f"{name}/boxes0"][-1]   # the root is made last
        sets = make_sets(name, rng, refs[0].scene, leaf_boxes, world_box)
        tables = {}
        for set_name in RW.SETS:
            s = sets[set_name]
            key = f"{name}/{set_name}"
            if "again" in s:   # rays of the free (0 .. N-1) and inside (N .. 2N-1) sets again: their positions, not their numbers
                out[key + "/again"] = s["again"].astype(np.uint16)
            else:
                RW.pack(out, key + "/o", s["o"])
                RW.pack(out, key + "/d", s["d"])
                out[key + "/factor"] = s["factor"].astype(np.uint8)
            for k in ("time", "tmin", "tmax"):
                RW.pack(out, f"{key}/{k}", s[k])
            for kind in RW.KINDS:
                rec = hit_record(refs[kind].scene, s["o"], s["d"] * RW.FACTORS[s["factor"]][:, None], s["time"], s["tmin"], s["tmax"])
                tables[f"{set_name}{kind}"] = rec
                share = float(np.mean(rec["hit"] != 0))
                say(f"{name} kind {kind} {set_name}: hits {share:.3f}, spheres {np.sum(rec['shape'] == 0)}, quads {np.sum(rec['shape'] == 1)}, "
                    f"media {np.sum(rec['shape'] == 2)}")
                assert 0.2 <= share <= 0.8, (name, set_name, share)
        RW.pack_rows(out, f"{name}/hits", RW.HIT_FIELDS, tables)

        # the step set and the paths of the inside rays
        fx = RW.Fixture(out)
        o, d, time = fx.step_rays(name)
        steps = {}
        for kind in RW.KINDS:
            s = refs[kind].scene.step(o, d, time, out["streams"])
            s["draws"] = draws_between(out["streams"], s["rng_state"])
            steps[f"{kind}"] = s
            seen_status |= set(s["status"].tolist())
            seen_kinds |= set(s["material"][s["status"] != 0].tolist())
            seen_faces |= set(s["front_face"][s["material"] == 2].tolist())
            metal_absorbs += int(np.sum((s["material"] == 1) & (s["status"] == 1)))
            say(f"{name} kind {kind} steps: status {np.bincount(s['status'], minlength=3)}, kinds {np.bincount(s['material'][s['status'] != 0], minlength=5)}, "
                f"medium {np.sum(s['flags'] & 1 != 0)}, noise {np.sum(s['flags'] & 2 != 0)}")
            assert set(s["status"].tolist()) == {0, 1, 2}, name
            radiance, exact = fold(refs[kind].scene, o[N:], d[N:], time[N:], out["streams"][N:])
            put(f"{name}/radiance", kind, radiance)
            put(f"{name}/radiance_exact", kind, exact)
            say(f"    radiance: {exact.sum()} of {N} paths met no medium and no noise")
            assert exact.sum() >= N // 8
        RW.pack_rows(out, f"{name}/steps", RW.STEP_FIELDS, steps)
        for kind in RW.KINDS:   # what the fixture gives back is what went in
            back = fx.steps(name, kind)
            assert all(np.array_equal(np.asarray(back[k]).view(np.uint8), np.asarray(steps[f"{kind}"][k]).astype(back[k].dtype).view(np.uint8))
                       for k in ("status", "emitted", "origin", "direction", "t", "rng_state"))
        for set_name in RW.SETS:
            got = fx.rays(name, set_name)
            want = (sets[set_name]["o"], sets[set_name]["d"] * RW.FACTORS[sets[set_name]["factor"]][:, None], sets[set_name]["time"],
                    sets[set_name]["tmin"], sets[set_name]["tmax"])
            assert all(np.array_equal(a.view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)) for a, b in zip(got, want))
    # over the worlds together (the free rays of one world alone need not find its small glass sphere from outside): all three
    # statuses, all five material kinds, both faces of the dielectric, a fuzzy metal that absorbs
    assert seen_status == {0, 1, 2} and seen_kinds == {0, 1, 2, 3, 4} and seen_faces == {0, 1} and metal_absorbs > 0
    return out


def main():
    if not R.available():
        sys.exit("build oracle/_ref first: make -C oracle ref")
    out = generate(verbose=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
