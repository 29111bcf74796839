"""Path advances (rt_scene_path_advance_device, PathBatch) against what they replace: the frames of profiles/r19_step.txt -- the
1200 x 800 centre rays of scene 7 (BVH and list) and of C2's list world (scene 11), one sample of 50 bounces, strict build.  One
GPU job, one frame per step, every step under its own time limit; each appends its lines to the file named last (default
profiles/r20_advance.txt):

  timeout -k 10 300 python profiles/advance_measure.py scene7 FILE && timeout -k 10 300 python profiles/advance_measure.py scene7list FILE &&
  timeout -k 10 400 python profiles/advance_measure.py c2 FILE

Per frame, library-seeded, torch tensors, best of three rounds after a warm-up, all in this one process:
  eager loop       the parent's loop around Scene.path_step as profiles/step_measure.py times it (its own function, run here)
  PathBatch        construction (two sets of ray tensors, workspace, radiance) and run(50) to a synchronize, for check_every 8, 0
                   and 1; the sum of the calls' kernel times (HIP events, a pass of its own in which every call waits)
  radiance         one Scene.radiance call, samples = 1, max_depth = 50, the same seed
Required, and the exit status says so: the batch's radiance equals the radiance call's bit for bit on every ray, and construction
plus run(50) at the default check_every is faster than the eager loop measured beside it.

A fourth argument `trace` runs one PathBatch.run(50) and nothing else, for a kernel trace that splits the kernels' time by name:
  rocprofv3 --kernel-trace --stats -d DIR -- python profiles/advance_measure.py scene7 FILE trace"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402
from step_measure import CONFIGS, DEPTH, H, ROUNDS, SEED, W, centre_rays, fold  # noqa: E402


def batch_run(scene, o, d, time0, check_every):
    """(radiance, seconds: construction, run to a synchronize)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batch = rt.PathBatch(scene, o, d, time=time0, seed=SEED)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    radiance = batch.run(DEPTH, check_every=check_every)
    torch.cuda.synchronize()
    return radiance, t1 - t0, time.perf_counter() - t1


def kernel_times(scene, o, d, time0):
    """The calls' kernel times: every advance with statistics (it waits), over the live rows as run(check_every=1) narrows them."""
    batch = rt.PathBatch(scene, o, d, time=time0, seed=SEED)
    seconds, rays, calls, capacity, first = 0.0, 0, 0, batch.n, None
    while calls < DEPTH and capacity > 0:
        st = batch.advance(1, capacity, stats=True)[0]
        first = first or st
        seconds, rays, calls, capacity = seconds + st.seconds, rays + st.rays, calls + 1, int(st.scattered)
    return seconds, rays, calls, first


def main(which, path, trace=False):
    name, scene_id, world = CONFIGS[which]
    scene = rt.builtin_scene(scene_id, world, W, H)
    o, d, time0 = centre_rays(scene)
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    if trace:
        radiance, _, _ = batch_run(scene, dev_o, dev_d, time0, 8)
        print(f"{name}: one PathBatch.run({DEPTH}), sum of the radiance {float(radiance.sum()):.6f}")
        return 0

    def radiance_call():
        torch.cuda.synchronize()
        begin = time.perf_counter()
        out, st = scene.radiance(dev_o, dev_d, time=time0, samples=1, max_depth=DEPTH, seed=SEED, want=("radiance",), stats=True)
        return out["radiance"], st, time.perf_counter() - begin

    fold(scene, dev_o, dev_d, time0)   # warm-up: uploads, code objects, allocations
    radiance_call()
    for every in (8, 0, 1):
        batch_run(scene, dev_o, dev_d, time0, every)
    best_fold = best_radiance = None
    best_batch, same = {}, True
    for _ in range(ROUNDS):
        got = fold(scene, dev_o, dev_d, time0)
        if best_fold is None or got[3][0] < best_fold[3][0]:
            best_fold = got
        got = radiance_call()
        if best_radiance is None or got[2] < best_radiance[2]:
            best_radiance = got
        for every in (8, 0, 1):
            radiance, construct, run = batch_run(scene, dev_o, dev_d, time0, every)
            same = same and bool(torch.equal(radiance.view(torch.int64), got[0].view(torch.int64)))
            if every not in best_batch or construct + run < sum(best_batch[every]):
                best_batch[every] = (construct, run)
    kernels, rays, calls, first = kernel_times(scene, dev_o, dev_d, time0)
    acc, fold_rays, steps, (whole, fold_kernels, fold_calls, caller), _ = best_fold
    radiance_value, st, radiance_wall = best_radiance
    same = same and bool(torch.equal(acc.view(torch.int64), radiance_value.view(torch.int64)))
    construct, run = best_batch[8]
    faster = construct + run < whole
    lines = [
        f"{name}: {W * H} rays, one sample of {DEPTH} bounces",
        f"  eager loop      whole loop {1e3 * whole:9.3f} ms, {steps} steps, {fold_rays} rays: step kernels {1e3 * fold_kernels:9.3f} ms, "
        f"calls {1e3 * fold_calls:9.3f} ms, the caller's masks, compaction and fold {1e3 * caller:9.3f} ms = {caller / whole:.2f} of the loop",
    ] + [
        f"  PathBatch       check_every {every}: construction {1e3 * best_batch[every][0]:8.3f} ms + run({DEPTH}) {1e3 * best_batch[every][1]:8.3f} ms"
        f" = {1e3 * sum(best_batch[every]):8.3f} ms; eager loop / this {whole / sum(best_batch[every]):6.2f}" for every in (8, 0, 1)
    ] + [
        f"  its kernels     {1e3 * kernels:9.3f} ms over {calls} calls of three launches, {rays} rays (each call timed by HIP events, waiting); "
        f"first call {1e3 * first.seconds:.3f} ms, {first.scattered} of {first.rays} rays scattered; {first.kernel_vgprs} VGPRs, {first.scratch_bytes} B scratch",
        f"  radiance        kernel {1e3 * st.seconds:9.3f} ms, call {1e3 * radiance_wall:9.3f} ms, {st.rays} rays; "
        f"{st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch",
        f"  PathBatch / radiance call: {(construct + run) / radiance_wall:.2f} wall, {kernels / st.seconds:.2f} kernels; "
        f"bit for bit the radiance call's on all {W * H} rays, every run: {same}; the same rays: {rays == st.rays}; "
        f"faster than the eager loop: {faster}",
    ]
    with open(path, "a") as f:
        for line in lines:
            print(line, flush=True)
            f.write(line + "\n")
    return 0 if same and faster else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r20_advance.txt"), len(sys.argv) > 3 and sys.argv[3] == "trace"))
