"""Path advances with light samples, measured: what PathBatch(direct="mis") costs a sample on scene 9 beside the eager MIS loop of
profiles/light_measure.py and beside Scene.radiance, and what it buys at equal wall time.

  timeout -k 10 900 python profiles/direct_measure.py [--output FILE]
  python profiles/direct_measure.py --one-sample      (two samples of the batch and nothing else: for a kernel trace)

Writes profiles/r23_direct.txt (or FILE): a header and every line it prints.  The frames of profiles/r21_lights.txt: 400 x 400
centre rays, depth 50, the reference 5000 samples a ray of plain Scene.radiance; the eager loop and Scene.radiance are run again
in this process.  One process, one GPU, strict build."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402
from light_measure import centre_rays, nee_radiance, scene9  # noqa: E402

DEPTH = 50
HEADER = """Path advances with light samples, measured (python profiles/direct_measure.py; one MI355X, one process, strict build).

Scene 9, 400 x 400 centre rays, depth 50.  The reference is 5000 samples a ray of plain Scene.radiance (ten calls of 500); against
it the RMSE over all rays and channels of Scene.radiance at N samples, of the eager MIS loop of INTEGRATION.md C1c (path_step,
sample_lights, light_pdf, occluded(*shadow_rays), eager torch between them) and of PathBatch(direct="mis").run(50) -- a new batch for
every sample, its allocation inside the clock -- each at the number of samples that takes about the wall time of Scene.radiance.
"""
_record = []


def say(line=""):
    print(line, flush=True)
    _record.append(line)


def batch_radiance(scene, o, d, time0, samples, seed, check_every=8, stats=None, direct="mis"):
    n = o.shape[0]
    total = torch.zeros((n, 3), dtype=torch.float64, device=o.device)
    for sample in range(samples):
        batch = rt.PathBatch(scene, o, d, time=time0, seed=seed, first_sequence=sample * n, direct=direct, strategy=1)
        if stats is None:
            total += batch.run(DEPTH, check_every=check_every)
            continue
        for bounce in range(DEPTH):   # measurements: every call waits and reports
            stats.extend(batch.advance(1, stats=True, sample=bounce < DEPTH - 1))
        total += batch.radiance
    return total / samples


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    w = h = 400
    scene = scene9(w, h)
    o, d, time0 = centre_rays(scene, w, h)
    if "--one-sample" in sys.argv:
        batch_radiance(scene, o, d, time0, 2, 6)
        torch.cuda.synchronize()
        return
    _record.append(HEADER)
    ref = torch.zeros_like(o)
    for part in range(10):   # 5000 samples a ray, in ten calls of 500 from streams of their own
        ref += scene.radiance(o, d, time=time0, samples=500, max_depth=DEPTH, seed=1, first_sequence=part * o.shape[0])["radiance"] / 10.0
        torch.cuda.synchronize()
        print(f"  reference: {500 * (part + 1)} samples", flush=True)

    def rmse(x):
        return float(torch.sqrt(torch.mean((x - ref) ** 2)))

    # one sample of each, after a warm-up
    nee_radiance(scene, o, d, time0, 1, DEPTH, 3, mis=True)
    batch_radiance(scene, o, d, time0, 1, 3)
    per_eager = min(timed(lambda: nee_radiance(scene, o, d, time0, 1, DEPTH, 3, mis=True))[1] for _ in range(3))
    per_batch = min(timed(lambda: batch_radiance(scene, o, d, time0, 1, 3))[1] for _ in range(3))
    per_batch_nowait = min(timed(lambda: batch_radiance(scene, o, d, time0, 1, 3, check_every=0))[1] for _ in range(3))
    batch_radiance(scene, o, d, time0, 1, 3, direct=None)
    per_plain_batch = min(timed(lambda: batch_radiance(scene, o, d, time0, 1, 3, direct=None))[1] for _ in range(3))
    scene.radiance(o, d, time=time0, samples=1, max_depth=DEPTH, seed=2)
    per_plain = min(timed(lambda: scene.radiance(o, d, time=time0, samples=16, max_depth=DEPTH, seed=2))[1] for _ in range(3)) / 16
    say(f"seconds a sample of {o.shape[0]} rays: Scene.radiance {per_plain:.4f}; the eager MIS loop {per_eager:.4f}; "
        f"PathBatch(direct=\"mis\").run(50) {per_batch:.4f} (count read every 8 bounces), {per_batch_nowait:.4f} (never read): "
        f"{per_eager / per_batch:.1f} x the eager loop's speed; the plain PathBatch.run(50) beside it {per_plain_batch:.4f}")
    for spp in (16, 64):
        plain, t_plain = timed(lambda: scene.radiance(o, d, time=time0, samples=spp, max_depth=DEPTH, seed=2)["radiance"])
        me = max(1, int(round(t_plain / per_eager)))
        eager, t_eager = timed(lambda: nee_radiance(scene, o, d, time0, me, DEPTH, 5, mis=True))
        mb = max(1, int(round(t_plain / per_batch)))
        fused, t_fused = timed(lambda: batch_radiance(scene, o, d, time0, mb, 7))
        say(f"mean radiance of the reference {float(ref.mean()):.4f}; Scene.radiance at {spp} samples against both MIS forms at equal time:")
        say(f"  Scene.radiance            {spp:4d} samples  {t_plain:7.3f} s  RMSE {rmse(plain):.4f}")
        say(f"  the eager loop with MIS   {me:4d} samples  {t_eager:7.3f} s  RMSE {rmse(eager):.4f}")
        say(f"  PathBatch(direct=\"mis\")   {mb:4d} samples  {t_fused:7.3f} s  RMSE {rmse(fused):.4f}")
        for name, x in (("Scene.radiance", plain), ("the eager loop with MIS", eager), ("PathBatch(direct=\"mis\")", fused)):
            err = (x - ref).abs().sum(dim=1)
            say(f"    {name:24s} mean {float(x.mean()):.4f}; median absolute error a ray {float(err.median()):.4f}, largest {float(err.max()):.2f}")
    # the calls of one sample, each waited for
    stats = []
    batch_radiance(scene, o, d, time0, 1, 9, stats=stats)
    rays = sum(s.rays for s in stats)
    say(f"one sample, every call waited for: {len(stats)} calls, {rays} rays stepped, {sum(s.shadow_rays for s in stats)} shadow rays cast, "
        f"{sum(s.shadow_reached for s in stats)} reached their lamp; {sum(s.seconds for s in stats):.4f} s in the calls' kernels (HIP events)")
    say(f"  first bounce: {stats[0].rays} rays, {stats[0].shadow_rays} shadow rays, {1e3 * stats[0].seconds:.3f} ms; "
        f"step-and-sample kernel {stats[0].kernel_vgprs} VGPRs, {stats[0].scratch_bytes} B scratch; "
        f"shadow kernel {stats[0].shadow_vgprs} VGPRs, {stats[0].shadow_scratch_bytes} B scratch")
    out = sys.argv[sys.argv.index("--output") + 1] if "--output" in sys.argv else os.path.join(ROOT, "profiles", "r23_direct.txt")
    with open(out, "w") as f:
        f.write("\n".join(_record) + "\n")


if __name__ == "__main__":
    main()
