"""Ray queries (rt_scene_intersect, Scene.intersect / Scene.occluded): the closest hit of caller-supplied rays against the feature
pass bit for bit (same search, same leaf tests, same hit record), against closed forms for what the feature pass cannot ask --
intervals, per-ray times, the far root, HitRecord U/V, the leaf that won -- and the plumbing: occlusion == hit, batch edges,
outputs left out, the torch path, the executable.  Every ray set is at most 32 x 24 rays."""
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
from query_helpers import bits, centre_rays, dot3, mixed_world, sphere_roots, uv_bound

pytestmark = pytest.mark.gpu

W, H = 32, 24
INF = float("inf")
ALL = ("t", "normal", "uv", "albedo", "leaf", "front_face", "material")


# ---- rays ----
def sphere_uv(n):
    """R/Sphere.h:74-81 on unit outward normals (N, 3): (u, v) as (N, 2)."""
    theta, phi = np.arccos(-n[:, 1]), np.arctan2(-n[:, 2], n[:, 0]) + np.pi
    return np.stack([phi / (2.0 * np.pi), theta / np.pi], axis=-1)


# ---- scenes ----
SCENES = {
    "mixed bvh": lambda: mixed_world(rt.Scene(), rt.Rng, 0, W / H), "mixed list": lambda: mixed_world(rt.Scene(), rt.Rng, 1, W / H),
    "scene 9 bvh": lambda: rt.builtin_scene(9, 0, W, H), "scene 9 list": lambda: rt.builtin_scene(9, 1, W, H),   # media that draw
    "scene 8 bvh": lambda: rt.builtin_scene(8, 0, W, H), "scene 8 list": lambda: rt.builtin_scene(8, 1, W, H),
}
HAS_MEDIA = {name: name.startswith("scene") for name in SCENES}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    scene = SCENES[name]()
    assert (scene.info()["n_media"] > 0) == HAS_MEDIA[name]
    return scene


@functools.lru_cache(maxsize=None)
def closest_of(name, variant=0):
    """Every output of the closest-hit query of the scene's centre rays, computed once and shared (nobody writes to it)."""
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    out = scene.intersect(o, d, time=time0, variant=variant, want=ALL + ("occluded",))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def closed_form_sphere():
    """The scene of test_sphere_depth_and_normal_equal_the_closed_form and what the issue states of its 768 centre rays."""
    bg_colour, centre, radius, colour = (0.2, 0.3, 0.9), (0.1, 0.05, -3.0), 0.8, (0.6, 0.4, 0.1)
    s = rt.Scene()
    s.SetWorld(s.HittableList([s.Sphere(centre, radius, s.Lambertian(colour))]))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 0.0, bg_colour)
    s.Commit()
    o, d, _, bg = centre_rays(s, W, H)
    near, far, rel_disc = sphere_roots(o, d, centre, radius)
    grazing = np.abs(rel_disc) <= 1e-9
    assert grazing.mean() <= 0.02 and not grazing.any(), "no centre ray of this set grazes the sphere"
    hits = np.isfinite(near)
    assert 0.33 < hits.mean() < 0.35
    assert 2.20 <= near[hits].min() and near[hits].max() <= 2.78 and 2.83 <= far[hits].min() and far[hits].max() <= 3.80
    return s, o, d, bg, np.asarray(centre), radius, colour, hits, near, far


# windows over the ray parameter, from the ranges above: (tmin, tmax) -> which root a hitting ray reports
WINDOWS = {"whole": (0.001, INF, "near"), "tmax 2.0": (0.001, 2.0, None), "tmin 2.8": (2.8, INF, "far"), "tmin 4.0": (4.0, INF, None)}


# ---- 1. against the feature pass ----
@pytest.mark.parametrize("name", sorted(SCENES))
def test_centre_rays_equal_the_feature_pass_bit_for_bit(name):
    scene = scene_of(name)
    o, d, _, _ = centre_rays(scene, W, H)
    film = rt.Film(W, H)
    film.render_features(scene, samples=0, seed=1984, variant=0)
    albedo, normal, depth = (p.reshape(W * H, -1) for p in film.features())
    depth = depth[:, 0]
    got = closest_of(name)
    hit = np.isfinite(got["t"])
    print(f"{name}: {hit.sum()} of {hit.size} rays hit, {np.sum(got['material'] == 4)} on an isotropic material")
    assert 0 < hit.sum() and np.array_equal(hit, depth > 0)
    if HAS_MEDIA[name]:
        assert np.sum(got["material"] == 4) > 0, "some ray ends inside a medium: the stream rule is exercised"
    assert np.array_equal(bits(got["normal"]), bits(normal))
    assert np.array_equal(bits(got["albedo"]), bits(albedo))
    want = got["t"][hit] * np.sqrt(dot3(d, d))[hit]
    rel = np.abs(want - depth[hit]) / depth[hit]
    print(f"    t |d| against depth: worst relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-15
    assert (got["leaf"][~hit] == -1).all() and (got["material"][~hit] == 255).all() and (got["front_face"][~hit] == 0).all()
    assert (got["leaf"][hit] >= 0).all() and (got["leaf"][hit] < scene.info()["n_leaves"]).all()


# ---- 2. closed forms and windows ----
def _check_window(out, window, variant):
    s, o, d, bg, centre, radius, colour, hits, near, far = closed_form_sphere()
    tmin, tmax, root = WINDOWS[window]
    t = out["t"]
    if root is None:
        assert np.isinf(t).all() and (t > 0).all(), "every ray misses"
        assert (out["leaf"] == -1).all() and (out["normal"] == 0).all() and (out["material"] == 255).all()
        assert np.array_equal(out["albedo"], np.broadcast_to(bg, out["albedo"].shape))
        return
    want_t = (near if root == "near" else far)[hits]
    assert np.array_equal(np.isfinite(t), hits)
    rel = np.abs(t[hits] - want_t) / want_t
    outward = ((o[hits] + want_t[:, None] * d[hits]) - centre) / radius
    want_n = outward if root == "near" else -outward
    err_n = np.abs(out["normal"][hits] - want_n)
    print(f"variant {variant}, {window}: t rel err {rel.max():.3g}, normal err {err_n.max():.3g}, {hits.sum()} hits")
    assert rel.max() <= 1e-12 and err_n.max() <= 1e-12
    assert (out["front_face"][hits] == (1 if root == "near" else 0)).all()
    err_uv = np.abs(out["uv"][hits] - sphere_uv(outward))   # HitRecord U, V come from the OUTWARD normal (R/Sphere.h:44,56)
    print(f"    uv err {err_uv.max():.3g} (bound {uv_bound(outward).min():.3g} .. {uv_bound(outward).max():.3g})")
    assert (err_uv <= uv_bound(outward)).all() and (out["uv"][~hits] == 0).all()
    assert (out["leaf"][hits] == 0).all() and (out["material"][hits] == 0).all()
    assert np.array_equal(out["albedo"][hits], np.broadcast_to(colour, out["albedo"][hits].shape))
    assert np.isinf(t[~hits]).all() and (out["normal"][~hits] == 0).all()
    assert np.array_equal(out["albedo"][~hits], np.broadcast_to(bg, out["albedo"][~hits].shape)), "a miss shows the background, exactly"


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_sphere_roots_equal_the_closed_form_in_every_window(variant):
    s, o, d = closed_form_sphere()[:3]
    alone = {}
    for window, (tmin, tmax, _) in WINDOWS.items():
        alone[window] = s.intersect(o, d, tmin=tmin, tmax=tmax, variant=variant)
        _check_window(alone[window], window, variant)
    # the same windows as per-ray arrays, mixed within one batch: ray k takes window k % 4
    names = list(WINDOWS)
    which = np.arange(W * H) % len(names)
    tmin = np.array([WINDOWS[names[w]][0] for w in which])
    tmax = np.array([WINDOWS[names[w]][1] for w in which])
    mixed = s.intersect(o, d, tmin=tmin, tmax=tmax, variant=variant)
    for w, window in enumerate(names):
        for key in ALL:
            assert np.array_equal(bits(mixed[key][which == w]), bits(alone[window][key][which == w])), (window, key)
    # one array and one scalar
    half = s.intersect(o, d, tmin=np.full(W * H, 2.8), variant=variant)
    assert all(np.array_equal(bits(half[key]), bits(alone["tmin 2.8"][key])) for key in ALL)


# ---- 3. a moving sphere at per-ray times ----
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_moving_sphere_follows_per_ray_times(world):
    c0, c1, radius = np.array((-0.5, 0.0, -3.0)), np.array((0.5, 0.25, -3.5)), 0.7
    s = rt.Scene()
    items = [s.MovingSphere(c0, c1, 0.0, 1.0, radius, s.Metal((0.8, 0.8, 0.8), 0.0)),
             s.Sphere((0.0, 0.0, -40.0), 1.0, s.Lambertian((0.5, 0.5, 0.5)))]   # far behind: never nearer than the mover
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, W / H, 0.0, 1.0, 0.0, 1.0)
    s.Commit()
    o1, d1, _, _ = centre_rays(s, 16, 16)
    shutter = (0.0, 0.25, 1.0)
    o, d = np.tile(o1, (3, 1)), np.tile(d1, (3, 1))
    times = np.repeat(shutter, len(o1))
    mover = int(np.flatnonzero(s.dump_leaves()[0] == 1)[0])
    for variant in (0, 1):
        out = s.intersect(o, d, times=times, variant=variant)
        seen = []
        for tm in shutter:
            centre = c0 + ((tm - 0.0) / (1.0 - 0.0)) * (c1 - c0)   # R/MovingSphere.h:51-52
            rays = times == tm
            near, _, rel_disc = sphere_roots(o[rays], d[rays], centre, radius)
            sure = np.abs(rel_disc) > 1e-9
            assert (~sure).mean() <= 0.02
            hit = np.isfinite(near) & sure
            on_mover = out["leaf"][rays] == mover
            assert np.array_equal(on_mover[sure], hit[sure]) and hit.sum() > 20
            t, n = out["t"][rays][hit], out["normal"][rays][hit]
            want_n = ((o[rays][hit] + near[hit, None] * d[rays][hit]) - centre) / radius
            rel, err_n = np.abs(t - near[hit]) / near[hit], np.abs(n - want_n)
            print(f"{world}, variant {variant}, time {tm}: t rel err {rel.max():.3g}, normal err {err_n.max():.3g}, {hit.sum()} hits")
            assert rel.max() <= 1e-12 and err_n.max() <= 1e-12
            assert (out["material"][rays][hit] == 1).all() and (out["front_face"][rays][hit] == 1).all()
            err_uv = np.abs(out["uv"][rays][hit] - sphere_uv(want_n))   # R/MovingSphere.h:70
            print(f"    uv err {err_uv.max():.3g}")
            assert (err_uv <= uv_bound(want_n)).all()
            seen.append(on_mover)
        assert not np.array_equal(seen[0], seen[2]), "the sphere moves across the frame between the shutter's ends"
        # one time for all rays is the scalar's business
        alone = s.intersect(o1, d1, time=0.25, variant=variant)
        assert all(np.array_equal(bits(alone[key]), bits(out[key][times == 0.25])) for key in ALL)


# ---- 4. quads and the instanced, rotated box ----
@pytest.mark.parametrize("world", ["bvh", "list"])
def test_quads_and_an_instanced_box(world):
    floor_c, wall_c, box_c = (0.25, 0.5, 0.125), (0.5, 0.25, 0.75), (0.75, 0.75, 0.25)
    quads = {"floor": ((-30, -1, -30), (60, 0, 0), (0, 0, 60)), "wall": ((-30, -1, -6), (60, 0, 0), (0, 30, 0))}
    s = rt.Scene()
    items = [s.Quad(*quads["floor"], s.Lambertian(floor_c)), s.Quad(*quads["wall"], s.Metal(wall_c, 0.1)),
             s.RotateY(s.Translate(s.MakeBox((-0.6, -1.0, -0.6), (0.6, 0.4, 0.6), s.Lambertian(box_c)), (0.3, 0.0, -2.5)), 25.0)]
    s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
    s.Camera((0, 0.6, 3), (0, 0, -2), (0, 1, 0), 50.0, W / H, 0.0, 1.0)
    s.Commit()
    o, d, time0, _ = centre_rays(s, W, H)
    out = s.intersect(o, d, time=time0)
    t, normal = out["t"], out["normal"]
    assert np.isfinite(t).all(), "floor and wall fill the frame"
    assert np.abs(np.linalg.norm(normal, axis=-1) - 1.0).max() <= 1e-15
    assert (dot3(normal, d) < 0).all(), "face() turns the normal against the ray"
    on = {name: (out["albedo"] == c).all(axis=-1) for name, c in (("floor", floor_c), ("wall", wall_c), ("box", box_c))}
    assert on["floor"].any() and on["wall"].any() and on["box"].sum() > 20 and (on["floor"] | on["wall"] | on["box"]).all()
    kinds, boxes = s.dump_leaves()
    point = o + t[:, None] * d
    for name, material in (("floor", 0), ("wall", 1), ("box", 0)):
        leaves = np.unique(out["leaf"][on[name]])
        assert len(leaves) == 1 and kinds[leaves[0]] == (3 if name == "box" else 2), name
        assert (out["material"][on[name]] == material).all(), "material kinds as built"
        lo, hi = boxes[leaves[0]][0::2], boxes[leaves[0]][1::2]
        assert ((point[on[name]] >= lo - 1e-9) & (point[on[name]] <= hi + 1e-9)).all(), "the hit lies in its leaf's box"
    for name, (q, u, v) in quads.items():
        q, u, v = (np.asarray(x, dtype=np.float64) for x in (q, u, v))
        n = np.cross(u, v)
        outward = (1.0 / np.sqrt(dot3(n, n))) * n   # R/Quad.h:33-37
        front = dot3(d[on[name]], outward) < 0
        assert np.array_equal(out["front_face"][on[name]] != 0, front), "FrontFace is the sign of n . d"
        assert front.all() == (name == "wall") and front.any() == (name == "wall"), "the camera is above the floor's back, in front of the wall"
        assert (normal[on[name]] == np.where(front[:, None], outward, -outward)).all(), "the plane's normal, exactly"
        w = n / dot3(n, n)
        ph = point[on[name]] - q
        alpha, beta = dot3(w, np.cross(ph, v)), dot3(w, np.cross(u, ph))   # R/Quad.h:74-97
        err = max(np.abs(out["uv"][on[name], 0] - alpha).max(), np.abs(out["uv"][on[name], 1] - beta).max())
        print(f"{world}, {name}: {on[name].sum()} hits, uv err {err:.3g}")
        assert err <= 1e-12 and (alpha >= 0).all() and (alpha <= 1).all() and (beta >= 0).all() and (beta <= 1).all()
    assert (out["front_face"][on["box"]] == 1).all(), "the box is seen from outside"
    st, ct = np.sin(np.radians(25.0)), np.cos(np.radians(25.0))
    faces = np.array([(0, 1, 0), (ct, 0, -st), (-ct, 0, st), (st, 0, ct), (-st, 0, -ct)])
    assert np.abs(normal[on["box"]][:, None, :] - faces[None]).max(axis=-1).min(axis=-1).max() <= 1e-15
    # U/V under the instance chain: the hit in the box's own space -- RotateY turns the world ray by -25 degrees (R/Instance.h:
    # 88-97), Translate then takes the offset off (R/Instance.h:43-45) -- and (alpha, beta) of the MakeBox face that was hit
    # (R/Instance.h:176-181: front, right, back, left, top), R/Quad.h:74-97
    lo, hi, offset = np.array((-0.6, -1.0, -0.6)), np.array((0.6, 0.4, 0.6)), np.array((0.3, 0.0, -2.5))
    dx, dy, dz = np.array((hi[0] - lo[0], 0, 0)), np.array((0, hi[1] - lo[1], 0)), np.array((0, 0, hi[2] - lo[2]))
    sides = {(0, 0, 1): ((lo[0], lo[1], hi[2]), dx, dy), (1, 0, 0): ((hi[0], lo[1], hi[2]), -dz, dy), (0, 0, -1): ((hi[0], lo[1], lo[2]), -dx, dy),
             (-1, 0, 0): ((lo[0], lo[1], lo[2]), dz, dy), (0, 1, 0): ((lo[0], hi[1], hi[2]), dx, -dz)}

    def turn(p):
        return np.stack([ct * p[:, 0] - st * p[:, 2], p[:, 1], st * p[:, 0] + ct * p[:, 2]], axis=-1)

    local_p, local_n = turn(point[on["box"]]) - offset, np.rint(turn(normal[on["box"]]))
    seen_sides = 0
    for axis, (q, u, v) in sides.items():
        mine = (local_n == np.array(axis)).all(axis=-1)
        if not mine.any():
            continue
        seen_sides += 1
        n = np.cross(u, v)
        w = n / dot3(n, n)
        ph = local_p[mine] - np.array(q)
        alpha, beta = dot3(w, np.cross(ph, v)), dot3(w, np.cross(u, ph))
        got_uv = out["uv"][on["box"]][mine]
        err = max(np.abs(got_uv[:, 0] - alpha).max(), np.abs(got_uv[:, 1] - beta).max())
        print(f"{world}, box side {axis}: {mine.sum()} hits, uv err {err:.3g}")
        assert err <= 1e-12 and alpha.min() > -1e-9 and alpha.max() < 1 + 1e-9 and beta.min() > -1e-9 and beta.max() < 1 + 1e-9
    assert seen_sides >= 2


# ---- 5. which leaf ----
def test_leaf_is_the_position_of_the_nearest_object_in_both_world_kinds():
    rng = np.random.default_rng(11)
    centres = np.array([(-2.4 + 0.6 * k, 0.2 + 0.5 * (k % 3), -4.0 - 0.7 * (k % 4)) for k in range(9)])
    radii = 0.4 + 0.05 * rng.integers(0, 3, 9)
    gaps = np.linalg.norm(centres[:, None] - centres[None], axis=-1) - (radii[:, None] + radii[None]) + 10.0 * np.eye(9)
    assert gaps.min() > 0.05, "the spheres are disjoint"
    ground = ((-20.0, -0.5, -20.0), (40.0, 0, 0), (0, 0, 40.0))
    found = {}
    for world in ("list", "bvh"):
        s = rt.Scene()
        m = s.Lambertian((0.5, 0.5, 0.5))
        items = [s.Sphere(c, float(r), m) for c, r in zip(centres, radii)] + [s.Quad(*ground, m)]
        assert len(set(items)) == len(items), "no handle twice"
        s.SetWorld(s.BvhNode(items) if world == "bvh" else s.HittableList(items))
        s.Camera((0, 1.0, 2.0), (0, 0.3, -4.0), (0, 1, 0), 45.0, W / H, 0.0, 1.0)
        s.Commit()
        o, d, time0, _ = centre_rays(s, W, H)
        # the analytically nearest object: 0..8 the spheres, 9 the ground, -1 nothing
        ts = np.full((10, len(o)), INF)
        sure = np.ones(len(o), dtype=bool)
        for k in range(9):
            near, _, rel_disc = sphere_roots(o, d, centres[k], radii[k])
            ts[k] = np.where(np.isfinite(near) & (near > 0.001), near, INF)
            sure &= np.abs(rel_disc) > 1e-9
        with np.errstate(divide="ignore"):
            tg = (-0.5 - o[:, 1]) / d[:, 1]
        pg = o + tg[:, None] * d
        ts[9] = np.where((tg > 0.001) & (np.abs(pg[:, 0]) < 20) & (np.abs(pg[:, 2]) < 20), tg, INF)
        nearest = np.where(np.isfinite(ts.min(axis=0)), ts.argmin(axis=0), -1)
        assert (~sure).mean() <= 0.02 and len(np.unique(nearest)) >= 8, "most objects are in sight"
        # object -> position in dump_leaves: a sphere's box is centre -+ radius, the ground is the one quad
        kinds, boxes = s.dump_leaves()
        assert len(kinds) == 10
        position = np.full(11, -1)
        for k in range(9):
            match = np.flatnonzero((kinds == 0) & (np.abs(boxes[:, 0::2] - (centres[k] - radii[k])).max(axis=1) < 1e-12))
            assert len(match) == 1
            position[k] = match[0]
        position[9] = np.flatnonzero(kinds == 2)[0]
        if world == "list":
            assert np.array_equal(position[:10], np.arange(10)), "a list keeps its order"
        else:
            assert not np.array_equal(position[:10], np.arange(10)), "the tree sorted its leaves"
        for variant in (0, 1):
            out = s.intersect(o, d, time=time0, variant=variant)
            assert np.array_equal(out["leaf"][sure], position[nearest][sure]), (world, variant)
            hit = out["leaf"] >= 0
            point = o[hit] + out["t"][hit, None] * d[hit]
            lo, hi = boxes[out["leaf"][hit]][:, 0::2], boxes[out["leaf"][hit]][:, 1::2]
            assert ((point >= lo - 1e-9) & (point <= hi + 1e-9)).all(), "the hit point lies in the reported leaf's box"
        inverse = np.full(10, -1)
        inverse[position[:10]] = np.arange(10)
        found[world] = np.where(hit, inverse[out["leaf"]], -1)
    assert np.array_equal(found["list"], found["bvh"]), "both world kinds see the same object"


# ---- 6. occlusion ----
@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_occluded_is_exactly_a_hit_of_the_closest_query(name, variant):
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    got = closest_of(name, variant)
    assert np.array_equal(got["occluded"] != 0, np.isfinite(got["t"])), "the closest-hit query's own flag"
    for tmin, tmax in ((0.001, INF), (0.001, 3.0), (2.5, INF)):
        closest = scene.intersect(o, d, time=time0, tmin=tmin, tmax=tmax, variant=variant, want=("t",))["t"]
        occluded, st = scene.occluded(o, d, time=time0, tmin=tmin, tmax=tmax, variant=variant, stats=True)
        print(f"{name}, variant {variant}, ({tmin}, {tmax}): {occluded.sum()} of {occluded.size} occluded, {st.kernel_vgprs} VGPRs")
        assert np.array_equal(occluded, np.isfinite(closest))
        assert st.rays == occluded.size and st.hits == occluded.sum()


@pytest.mark.parametrize("variant", [0, 1], ids=["strict", "fast"])
def test_occluded_follows_the_windows_of_the_sphere(variant):
    s, o, d, _, _, _, _, hits = closed_form_sphere()[:8]
    for window, (tmin, tmax, root) in WINDOWS.items():
        occluded = s.occluded(o, d, tmin=tmin, tmax=tmax, variant=variant)
        assert np.array_equal(occluded, hits if root else np.zeros_like(hits)), window
    names = list(WINDOWS)
    which = np.arange(W * H) % len(names)
    occluded = s.occluded(o, d, tmin=np.array([WINDOWS[names[w]][0] for w in which]), tmax=np.array([WINDOWS[names[w]][1] for w in which]),
                          variant=variant)
    assert np.array_equal(occluded, hits & np.isin(which, [0, 2]))


# ---- 7. batch boundaries and order ----
GUARD = {"float64": 12345.678, "int32": -77, "uint8": 0xAB}


def _device_query(scene, o, d, count, time, mode=0, first_sequence=0, variant=0):
    """rt_scene_intersect_device on the first `count` rays with every output one element longer than the call may write: returns
    the outputs (numpy, the guard cut off) after checking that the guard words still hold their value."""
    dev_o, dev_d = torch.from_numpy(o[:count].copy()).cuda(), torch.from_numpy(d[:count].copy()).cuda()
    outs = {}
    for name, (dtype, tail) in _lib.QUERY_OUTPUTS.items():
        per_ray = int(np.prod(tail)) if tail else 1
        outs[name] = torch.full((count * per_ray + 1,), GUARD[dtype], dtype=getattr(torch, dtype), device="cuda")
    p = _lib.QueryParams(count, 0.001, INF, time, 1984, first_sequence, mode, variant, 0, None)
    rays = _lib.QueryRays(dev_o.data_ptr(), dev_d.data_ptr(), None, None, None)
    hits = _lib.QueryHits(**{name: a.data_ptr() for name, a in outs.items()})
    torch.cuda.synchronize()
    status = api.lib().rt_scene_intersect_device(scene._p, C.byref(p), C.byref(rays), C.byref(hits), None)
    assert status == 0, api.lib().rt_last_error().decode()
    result = {}
    for name, (dtype, tail) in _lib.QUERY_OUTPUTS.items():
        a = outs[name].cpu().numpy()
        assert a[-1] == np.dtype(dtype).type(GUARD[dtype]), f"{name}: the word behind ray {count - 1} was written"
        result[name] = a[:-1].reshape((count,) + tail)
    return result


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_batch_edges_write_exactly_their_rays(count):
    for name in ("mixed bvh", "mixed list"):
        scene = scene_of(name)
        o, d, time0, _ = centre_rays(scene, W, H)
        whole = closest_of(name)
        got = _device_query(scene, o, d, count, time0)
        for key in ALL + ("occluded",):
            assert np.array_equal(bits(got[key]), bits(whole[key][:count])), (name, key)
        occlusion = _device_query(scene, o, d, count, time0, mode=1)
        assert np.array_equal(occlusion["occluded"], whole["occluded"][:count])
        for key in ALL:   # an occlusion query writes nothing else
            assert (occlusion[key] == np.dtype(_lib.QUERY_OUTPUTS[key][0]).type(GUARD[_lib.QUERY_OUTPUTS[key][0]])).all(), key


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_statistics_count_the_hits_and_leave_the_outputs_alone(name):
    """The closest-hit query with statistics (two events and a counter word around the kernel) against the plain launch: the same
    outputs bit for bit.  100 rays are one full wave and a ragged one for the count of one atomic per wave."""
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    o, d = o[:100].copy(), d[:100].copy()
    plain = scene.intersect(o, d, time=time0, variant=0, want=ALL + ("occluded",))
    counted, st = scene.intersect(o, d, time=time0, variant=0, want=ALL + ("occluded",), stats=True)
    print(f"{name}: {st.hits} of {st.rays} rays hit, {st.kernel_vgprs} VGPRs, {st.seconds * 1e3:.3f} ms")
    for key in ALL + ("occluded",):
        assert np.array_equal(bits(counted[key]), bits(plain[key])), key
        assert np.array_equal(bits(plain[key]), bits(closest_of(name)[key][:100])), key
    assert st.rays == 100 and st.hits == np.isfinite(plain["t"]).sum()
    assert 0 < st.hits, "a counter that stayed at its memset would pass the line above if every ray missed"
    assert st.kernel_vgprs > 0 and st.seconds > 0


@pytest.mark.parametrize("name", ["mixed bvh", "mixed list"])
def test_permuted_rays_give_permuted_results(name):
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    order = np.random.default_rng(3).permutation(len(o))
    whole = closest_of(name)
    got = scene.intersect(np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), time=time0)
    for key in ALL:
        assert np.array_equal(bits(got[key]), bits(whole[key][order])), key


@pytest.mark.parametrize("name", ["scene 9 bvh", "scene 9 list"])
def test_a_split_batch_continues_the_streams(name):
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    whole = closest_of(name)
    split = 301
    first = scene.intersect(o[:split].copy(), d[:split].copy(), time=time0)
    second = scene.intersect(o[split:].copy(), d[split:].copy(), time=time0, first_sequence=split)
    for key in ALL:
        assert np.array_equal(bits(np.concatenate([first[key], second[key]])), bits(whole[key])), key
    restarted = scene.intersect(o[split:].copy(), d[split:].copy(), time=time0)   # without it the media draw from other streams
    assert not np.array_equal(bits(restarted["t"]), bits(whole["t"][split:]))
    assert np.array_equal(scene.occluded(o[split:].copy(), d[split:].copy(), time=time0, first_sequence=split), np.isfinite(whole["t"][split:]))


# ---- 8. outputs left out ----
@pytest.mark.parametrize("name", ["mixed bvh", "scene 9 list"])
def test_each_output_alone_is_that_output_among_all(name):
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    whole = closest_of(name)
    for key in ALL + ("occluded",):
        alone = scene.intersect(o, d, time=time0, want=(key,))
        assert list(alone) == [key]
        assert np.array_equal(bits(alone[key]), bits(whole[key])), key


# ---- 9. torch ----
def test_torch_tensors_are_read_in_place_and_leave_films_alone():
    name = "scene 8 bvh"
    scene = scene_of(name)
    o, d, time0, _ = centre_rays(scene, W, H)
    film = rt.Film(W, H)
    before_stats = film.render(scene, 2, variant=0)
    before = film.download()
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    times = torch.full((len(o),), time0, dtype=torch.float64, device="cuda")
    out = scene.intersect(dev_o, dev_d, times=times, want=ALL + ("occluded",))
    whole = closest_of(name)
    for key, a in out.items():
        assert isinstance(a, torch.Tensor) and a.device == dev_o.device
        assert np.array_equal(bits(a.cpu().numpy()), bits(whole[key])), key
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # the current stream is the one the query runs on (and waits for)
        occluded = scene.occluded(dev_o, dev_d, time=time0)
    assert isinstance(occluded, torch.Tensor) and occluded.dtype == torch.bool
    assert np.array_equal(occluded.cpu().numpy(), whole["occluded"] != 0)
    for bad in (dev_o.float(), dev_o.t().contiguous().t(), torch.from_numpy(o)):
        with pytest.raises(rt.RtowError):
            scene.intersect(bad, dev_d)
    with pytest.raises(rt.RtowError):
        scene.intersect(dev_o, d)   # a numpy array beside a tensor
    after_stats = film.render(scene, 2, variant=0)
    assert np.array_equal(bits(film.download()), bits(before)), "the same frame before and after the queries"
    assert (before_stats.rays, before_stats.samples, before_stats.kernel_kind, before_stats.lds_bytes) == \
        (after_stats.rays, after_stats.samples, after_stats.kernel_kind, after_stats.lds_bytes)


# ---- 10. the executable ----
@pytest.mark.parametrize("scene_id, pixel", [(7, (13, 9)), (8, (16, 12))])
def test_rtow_pick_prints_what_the_api_returns(scene_id, pixel):
    i, j = pixel
    exe = os.path.join(os.path.dirname(rt.library_path()), "rtow")
    run = subprocess.run([exe, "--scene", str(scene_id), "--width", str(W), "--height", str(H), "--variant", "strict", "--pick", f"{i},{j}"],
                         check=True, cwd=ROOT, timeout=120, capture_output=True, text=True)
    lines = [line for line in run.stdout.splitlines() if line.startswith("pick ")]
    assert len(lines) == 1 and run.stdout.count("\n") == 1, run.stdout
    words = lines[0].split()
    assert words[1] == f"{i},{j}:" and [words[k] for k in (2, 4, 6, 8, 12, 16)] == ["leaf", "material", "t", "point", "normal", "albedo"]
    scene = rt.builtin_scene(scene_id, 0, W, H)
    o, d, time0, _ = centre_rays(scene, W, H)
    k = j * W + i
    out = scene.intersect(o[k:k + 1].copy(), d[k:k + 1].copy(), time=time0, first_sequence=k)
    assert np.isfinite(out["t"][0]), "the picked pixel shows an object"
    assert int(words[3]) == out["leaf"][0]
    assert words[5] == ("lambertian", "metal", "dielectric", "diffuse_light", "isotropic")[out["material"][0]]
    assert float(words[7]) == out["t"][0]
    assert [float(x) for x in words[9:12]] == list(o[k] + out["t"][0] * d[k])
    assert [float(x) for x in words[13:16]] == list(out["normal"][0])
    assert [float(x) for x in words[17:20]] == list(out["albedo"][0])


# ---- strict against fast ----
def test_strict_and_fast_agree_where_they_report_the_same_leaf():
    """Contraction may decide a comparison the other way (a ray that grazes, two surfaces at nearly one t; in a medium the draw that
    follows moves with it): where the two builds name the same leaf, t agrees to 1e-12 relative; how often they name another is
    printed, not asserted (profiles/r11_query.txt has the figure of one run)."""
    total = differ = 0
    for name in sorted(SCENES):
        strict, fast = closest_of(name, 0), closest_of(name, 1)
        same = strict["leaf"] == fast["leaf"]
        hit = same & (strict["leaf"] >= 0)
        rel = np.abs(strict["t"][hit] - fast["t"][hit]) / strict["t"][hit]
        print(f"{name}: the leaf differs on {np.sum(~same)} of {same.size} rays; same leaf: worst relative t difference {rel.max():.3g}")
        total, differ = total + same.size, differ + int(np.sum(~same))
        assert rel.max() <= 1e-12, name
    print(f"share of rays whose leaf differs between the builds: {differ} of {total} = {differ / total:.5f}")
