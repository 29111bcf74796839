"""Light sampling queries, measured: what sample_lights and light_pdf cost beside an occlusion query of the same count, and what
next-event estimation buys on scene 9 at equal wall time.

  timeout -k 10 900 python profiles/light_measure.py [--skip-frames] [--output FILE]

Writes profiles/r21_lights.txt (or FILE): a header and every line it prints.

1. 960 000 points (1200 x 800 first hits of the centre rays, torch tensors, strict build): sample_lights with every output, with
   direction / distance / pdf alone, light_pdf along the sampled directions, and the occlusion query of the shadow rays, best of
   five rounds after a warm-up, wall clock around the synchronous call and the kernel's own HIP-event time -- on scene 9 (one lamp)
   and on a world of kLightLdsRows + 1 lamps (an emissive mesh; one row beyond what a workgroup stages).
2. Scene 9, 400 x 400 centre rays: the RMSE against 5000 samples a ray of plain Scene.radiance, of Scene.radiance at N samples and of
   the next-event loop of INTEGRATION.md C1c at the number of samples that takes about the same wall time.  One process, one GPU."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402
from raytracinginoneweekendincuda_amd import _lib  # noqa: E402

ROUNDS = 5
HEADER = """Light sampling queries, measured (python profiles/light_measure.py; one MI355X, one process, strict build, torch tensors in place).

1. What the calls cost.  960 000 points: the first hits of the 1200 x 800 centre rays (Scene.path_step), the streams the step left.
Best of five rounds after a warm-up; "wall" is the clock around the synchronous call (launch, kernel, stream synchronisation),
"kernel" the call's own HIP events.  The occlusion query casts the shadow rays of those samples, occluded(*shadow_rays(...)).
"""
FRAMES = """
2. What next-event estimation buys on scene 9.  400 x 400 centre rays, depth 50.  The reference is 5000 samples a ray of plain
Scene.radiance (ten calls of 500); against it the RMSE over all rays and channels of Scene.radiance at N samples, and of the
next-event loop of INTEGRATION.md C1c (path_step, sample_lights, occluded(*shadow_rays), eager torch between them) at the number of
samples that takes about the same wall time -- once dropping the lamps that scattered rays find after a diffuse bounce, once keeping
both and weighting them by the balance heuristic (light_pdf, rt.scatter_pdf).
"""
_record = []


def say(line=""):
    print(line, flush=True)
    _record.append(line)


def centre_rays(scene, w, h):
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(w) + 0.5) / w)[None, :, None]
    v = ((np.arange(h) + 0.5) / h)[:, None, None]
    d = (((llc + u * hor) + v * ver) - origin).reshape(-1, 3)
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(origin, d.shape))).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda(), float(cam[25])


def scene9(w, h):
    with np.load(os.path.join(ROOT, "tests", "golden", "earthmap_stb.npz")) as g:
        return rt.builtin_scene(9, 0, w, h, earth=np.ascontiguousarray(g["bytes"]))


def best(call):
    call()
    torch.cuda.synchronize()
    wall, event, st = [], [], None
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        _, st = call()
        wall.append(time.perf_counter() - t0)
        event.append(st.seconds)
    return min(wall), min(event), st


def costs(name, scene, w, h):
    o, d, time0 = centre_rays(scene, w, h)
    hit = scene.path_step(o, d, time=time0, want=("status", "origin", "normal", "material", "rng_state"))
    n = o.shape[0]
    pts, nrm, mat, rng = hit["origin"], hit["normal"], hit["material"], hit["rng_state"]
    ls = scene.sample_lights(pts, nrm, mat, None, rng, time=time0)
    shadow = scene.shadow_rays(pts, ls["direction"].contiguous(), ls["distance"])
    runs = {
        "sample_lights, every output": lambda: scene.sample_lights(pts, nrm, mat, None, rng, time=time0, stats=True),
        "sample_lights, direction distance pdf": lambda: scene.sample_lights(pts, None, None, None, rng, time=time0, want=("direction", "distance", "pdf"), stats=True),
        "light_pdf along the samples": lambda: scene.light_pdf(pts, ls["direction"], time=time0, stats=True),
        "occluded(*shadow_rays)": lambda: scene.occluded(*shadow, time=time0, stats=True),
    }
    say(f"{name}: {n} points, {scene.info()['n_lights']} lights, {float((ls['pdf'] > 0).double().mean()):.3f} valid samples")
    for k, call in runs.items():
        wall, event, st = best(call)
        say(f"  {k:40s} wall {1e3 * wall:8.3f} ms = {n / wall * 1e-6:7.1f} M/s; kernel {1e3 * event:8.3f} ms = {n / event * 1e-6:8.1f} M/s, "
              f"{st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch")


def nee_radiance(scene, o, d, time0, samples, max_depth, seed, mis=False):
    """The loop of INTEGRATION.md C1c: path_step, sample_lights at the hit, occluded(*shadow_rays), and what the next step emits
    dropped after a Lambertian or isotropic bounce (the light samples have counted it) -- or, with ``mis``, both kept and weighted
    by the balance heuristic through light_pdf and rt.scatter_pdf."""
    n = o.shape[0]
    total = torch.zeros((n, 3), dtype=torch.float64, device=o.device)
    for sample in range(samples):
        ids = torch.arange(n, device=o.device)
        ro, rd, thr, rng = o, d, torch.ones((n, 3), dtype=torch.float64, device=o.device), None
        counted = torch.zeros(n, dtype=torch.bool, device=o.device)   # did the previous bounce sample the lights?
        for depth in range(max_depth):
            st = scene.path_step(ro, rd, time=time0, rng_state=rng, seed=seed, first_sequence=sample * n,
                                 want=("status", "emitted", "attenuation", "origin", "direction", "normal", "material", "rng_state"))
            lamp = (st["status"] == 1) & (st["material"] == 3)
            if mis and depth > 0:   # the lamp a scattered ray found: p_s / (p_s + p_l), 1 after a specular bounce
                p_l = scene.light_pdf(ro, rd, time=time0)["pdf"]
                keep = torch.where(lamp & counted, p_s / (p_s + p_l), torch.ones_like(p_l))
            else:
                keep = (~(lamp & counted)).double()
            total.index_add_(0, ids, thr * st["emitted"] * keep[:, None])
            go = st["status"] == 2
            if not bool(go.any()):
                break
            ids, thr = ids[go], thr[go] * st["attenuation"][go]
            ro, rd, nrm, mat = (st[k][go].contiguous() for k in ("origin", "direction", "normal", "material"))
            rng = st["rng_state"].view(torch.int32)[go].contiguous()   # (torch indexes no uint32)
            ls = scene.sample_lights(ro, nrm, mat, None, rng, time=time0, want=("direction", "distance", "scatter_pdf", "contribution", "rng_state"))
            # (scene 9 is full of fog: a medium answers a shadow ray from the query's own stream, curand_init(seed, k + first_sequence,
            # 0) -- a stream of its own for every call, or row k would meet the same fog in every sample and at every bounce)
            vis = ~scene.occluded(*scene.shadow_rays(ro, ls["direction"], ls["distance"]), time=time0, seed=seed + 1000,
                                  first_sequence=(sample * max_depth + depth) * n)
            direct = thr * ls["contribution"] * vis[:, None]
            if mis:   # the light sample: p_l / (p_l + p_s), p_l the mixture over all lamps
                q_l = scene.light_pdf(ro, ls["direction"], time=time0)["pdf"]
                q_s = ls["scatter_pdf"]
                direct = direct * torch.where(q_l + q_s > 0, q_l / (q_l + q_s), torch.zeros_like(q_l))[:, None]
                p_s = rt.scatter_pdf(mat, nrm, rd / torch.linalg.norm(rd, dim=1, keepdim=True))
            total.index_add_(0, ids, direct)
            rng = ls["rng_state"]
            counted = (mat == 0) | (mat == 4)
    return total / samples


def frames():
    w = h = 400
    scene = scene9(w, h)
    o, d, time0 = centre_rays(scene, w, h)
    ref = torch.zeros_like(o)
    for part in range(10):   # 5000 samples a ray, in ten calls of 500 from streams of their own
        ref += scene.radiance(o, d, time=time0, samples=500, max_depth=50, seed=1, first_sequence=part * o.shape[0])["radiance"] / 10.0
        torch.cuda.synchronize()
        print(f"  reference: {500 * (part + 1)} samples", flush=True)

    def rmse(x):
        return float(torch.sqrt(torch.mean((x - ref) ** 2)))

    for spp in (16, 64):
        scene.radiance(o, d, time=time0, samples=1, max_depth=50, seed=2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain = scene.radiance(o, d, time=time0, samples=spp, max_depth=50, seed=2)["radiance"]
        torch.cuda.synchronize()
        t_plain = time.perf_counter() - t0
        nee_radiance(scene, o, d, time0, 1, 50, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nee_radiance(scene, o, d, time0, 1, 50, 3)
        torch.cuda.synchronize()
        per_sample = time.perf_counter() - t0
        m = max(1, int(round(t_plain / per_sample)))
        t0 = time.perf_counter()
        nee = nee_radiance(scene, o, d, time0, m, 50, 4)
        torch.cuda.synchronize()
        t_nee = time.perf_counter() - t0
        nee_radiance(scene, o, d, time0, 1, 50, 3, mis=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nee_radiance(scene, o, d, time0, 1, 50, 3, mis=True)
        torch.cuda.synchronize()
        per_mis = time.perf_counter() - t0
        mm = max(1, int(round(t_plain / per_mis)))
        t0 = time.perf_counter()
        both = nee_radiance(scene, o, d, time0, mm, 50, 5, mis=True)
        torch.cuda.synchronize()
        t_mis = time.perf_counter() - t0
        say(f"mean radiance of the reference {float(ref.mean()):.4f}; Scene.radiance at {spp} samples against the loop at equal time:")
        say(f"  Scene.radiance      {spp:4d} samples  {t_plain:7.3f} s  RMSE {rmse(plain):.4f}")
        say(f"  next-event loop     {m:4d} samples  {t_nee:7.3f} s  RMSE {rmse(nee):.4f}   (one sample of the loop: {per_sample:.3f} s)")
        say(f"  the loop with MIS   {mm:4d} samples  {t_mis:7.3f} s  RMSE {rmse(both):.4f}   (one sample of the loop: {per_mis:.3f} s)")
        for name, x in (("Scene.radiance", plain), ("next-event loop", nee), ("the loop with MIS", both)):
            err = (x - ref).abs().sum(dim=1)
            say(f"    {name:18s} mean {float(x.mean()):.4f}; median absolute error a ray {float(err.median()):.4f}, largest {float(err.max()):.2f}")


def main():
    from light_worlds import many_lights_world
    _record.append(HEADER)
    costs("scene 9 (bvh)", scene9(1200, 800), 1200, 800)
    costs(f"{_lib.light_lds_rows() + 1} lamps (list)", many_lights_world(_lib.light_lds_rows() + 1)[0], 1200, 800)
    if "--skip-frames" not in sys.argv:
        _record.append(FRAMES)
        frames()
    out = sys.argv[sys.argv.index("--output") + 1] if "--output" in sys.argv else os.path.join(ROOT, "profiles", "r21_lights.txt")
    with open(out, "w") as f:
        f.write("\n".join(_record) + "\n")


if __name__ == "__main__":
    main()
