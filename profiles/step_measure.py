"""Path steps (rt_scene_path_step) as a caller's integrator uses them: the 1200 x 800 centre rays of scene 7 (BVH and list) and of
C2's list world (scene 11), one sample of 50 bounces, folded by steps in torch and once more as one Scene.radiance call.  One GPU
job, one frame per step, every step under its own time limit; each appends its lines to the file named last (default
profiles/r19_step.txt):

  timeout -k 10 200 python profiles/step_measure.py scene7 FILE && timeout -k 10 200 python profiles/step_measure.py scene7list FILE &&
  timeout -k 10 300 python profiles/step_measure.py c2 FILE

Per frame, strict build, library-seeded, torch tensors (the device calls: no copies), best of three rounds after a warm-up:
  first step       the step kernel on all rays: its HIP-event time, registers and scratch
  fold by steps    the loop of INTEGRATION.md "an integrator of your own" -- step the live rays, acc += thr * emitted where the path
                   ends, thr *= attenuation and keep the rays where it goes on -- until no ray is live or 50 steps are done: wall
                   time of the whole loop, the sum of the step kernels' HIP-event times, the wall time of the calls (launch, wait,
                   statistics, output allocation) and of the caller's part between them (masks, compaction, fold; torch on the
                   GPU, timed to a synchronize)
  radiance         one Scene.radiance call, samples = 1, max_depth = 50, the same seed: its kernel's HIP-event time and its wall time
The fold's result is compared with the radiance call's bit for bit, and its steps with the call's rays."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

W, H, DEPTH, ROUNDS, SEED = 1200, 800, 50, 3, 1984
CONFIGS = {"scene7": ("scene 7 (bvh)", 7, 0), "scene7list": ("scene 7 (list)", 7, 1), "c2": ("C2 (scene 11, list)", 11, 1)}
WANT = ("status", "emitted", "attenuation", "origin", "direction", "time", "rng_state")


def centre_rays(scene):
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(W) + 0.5) / W)[None, :, None]
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    d = (((llc + u * hor) + v * ver) - origin).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d), float(cam[25])


def fold(scene, o, d, time0):
    """(acc, rays stepped, steps, seconds: whole loop / kernels / calls / caller's part, the first step's statistics)"""
    n = o.shape[0]
    acc = torch.zeros((n, 3), dtype=torch.float64, device=o.device)
    thr = torch.ones_like(acc)              # of the live rays, compact like them
    live = torch.arange(n, device=o.device)
    tm = state = first = None
    rays = steps = 0
    kernels = calls = caller = 0.0
    torch.cuda.synchronize()
    begin = time.perf_counter()
    for _ in range(DEPTH):
        t0 = time.perf_counter()
        out, st = scene.path_step(o, d, times=tm, rng_state=state, time=time0, seed=SEED, want=WANT, stats=True)
        t1 = time.perf_counter()
        goes_on = out["status"] == 2
        ends = ~goes_on
        where = live[ends]
        product = thr[ends] * out["emitted"][ends]
        acc[where] = acc[where] + product
        thr = thr[goes_on] * out["attenuation"][goes_on]
        live = live[goes_on]
        o, d, tm, state = out["origin"][goes_on], out["direction"][goes_on], out["time"][goes_on], out["rng_state"].view(torch.int32)[goes_on]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        first = st if first is None else first
        rays, steps = rays + st.rays, steps + 1
        kernels, calls, caller = kernels + st.seconds, calls + (t1 - t0), caller + (t2 - t1)
        if live.numel() == 0:
            break
    return acc, rays, steps, (time.perf_counter() - begin, kernels, calls, caller), first


def main(which, path):
    name, scene_id, world = CONFIGS[which]
    scene = rt.builtin_scene(scene_id, world, W, H)
    o, d, time0 = centre_rays(scene)
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()

    def radiance():
        torch.cuda.synchronize()
        begin = time.perf_counter()
        out, st = scene.radiance(dev_o, dev_d, time=time0, samples=1, max_depth=DEPTH, seed=SEED, want=("radiance",), stats=True)
        return out["radiance"], st, time.perf_counter() - begin

    fold(scene, dev_o, dev_d, time0)   # warm-up: uploads, code objects, allocations
    radiance()
    best_fold = best_radiance = None
    for _ in range(ROUNDS):
        got = fold(scene, dev_o, dev_d, time0)
        if best_fold is None or got[3][0] < best_fold[3][0]:
            best_fold = got
        got = radiance()
        if best_radiance is None or got[1].seconds < best_radiance[1].seconds:
            best_radiance = got
    acc, rays, steps, (whole, kernels, calls, caller), first = best_fold
    radiance_value, st, radiance_wall = best_radiance
    same = bool(torch.equal(acc.view(torch.int64), radiance_value.view(torch.int64)))
    lines = [
        f"{name}: {W * H} rays, one sample of {DEPTH} bounces",
        f"  first step      kernel {1e3 * first.seconds:9.3f} ms, {first.scattered} of {first.rays} rays scattered; "
        f"{first.kernel_vgprs} VGPRs, {first.scratch_bytes} B scratch",
        f"  fold by steps   whole loop {1e3 * whole:9.3f} ms, {steps} steps, {rays} rays: step kernels {1e3 * kernels:9.3f} ms, "
        f"calls {1e3 * calls:9.3f} ms, the caller's masks, compaction and fold {1e3 * caller:9.3f} ms = {caller / whole:.2f} of the loop",
        f"  radiance        kernel {1e3 * st.seconds:9.3f} ms, call {1e3 * radiance_wall:9.3f} ms, {st.rays} rays; "
        f"{st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch",
        f"  fold / radiance: {whole / radiance_wall:.2f} wall, {kernels / st.seconds:.2f} kernels; "
        f"the fold is the radiance bit for bit: {same}, the same rays: {rays == st.rays}",
    ]
    with open(path, "a") as f:
        for line in lines:
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r19_step.txt"))
