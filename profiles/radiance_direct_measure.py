"""Radiance queries with light samples, measured: what a sample of Scene.radiance(direct="mis") costs on scene 9 beside
PathBatch(direct="mis").run(50) and beside plain Scene.radiance, all in one run, and what it buys at equal wall time.

  timeout -k 10 900 python profiles/radiance_direct_measure.py [--output FILE]
  python profiles/radiance_direct_measure.py --one-call      (one call of two samples and nothing else: for a kernel trace)

Writes profiles/r24_radiance_direct.txt (or FILE): a header and every line it prints.  The frames of profiles/r23_direct.txt: 400 x
400 centre rays, depth 50, the reference 5000 samples a ray of plain Scene.radiance.  One process, one GPU, strict build."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from direct_measure import DEPTH, batch_radiance, timed  # noqa: E402
from light_measure import centre_rays, scene9  # noqa: E402

HEADER = """Radiance queries with light samples, measured (python profiles/radiance_direct_measure.py; one MI355X, one process, strict build).

Scene 9, 400 x 400 centre rays, depth 50.  The reference is 5000 samples a ray of plain Scene.radiance (ten calls of 500); against
it the RMSE over all rays and channels of Scene.radiance at N samples, of Scene.radiance(direct="mis") -- one launch, all samples --
and of PathBatch(direct="mis").run(50) -- a new batch for every sample, its allocation inside the clock -- each at the number of
samples that takes about the wall time of Scene.radiance.  Every time below is of this run.
"""
_record = []


def say(line=""):
    print(line, flush=True)
    _record.append(line)


def main():
    w = h = 400
    scene = scene9(w, h)
    o, d, time0 = centre_rays(scene, w, h)

    def mis(samples, seed, stats=False):
        return scene.radiance(o, d, time=time0, samples=samples, max_depth=DEPTH, seed=seed, direct="mis", strategy=1, stats=stats)

    def plain(samples, seed):
        return scene.radiance(o, d, time=time0, samples=samples, max_depth=DEPTH, seed=seed)

    if "--one-call" in sys.argv:
        mis(2, 6)
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

    # a sample of each, after a warm-up, the three beside one another
    mis(1, 3)
    batch_radiance(scene, o, d, time0, 1, 3)
    plain(1, 2)
    per_mis_1 = min(timed(lambda: mis(1, 3))[1] for _ in range(3))
    per_mis = min(timed(lambda: mis(16, 3))[1] for _ in range(3)) / 16
    per_batch = min(timed(lambda: batch_radiance(scene, o, d, time0, 1, 3))[1] for _ in range(3))
    per_plain = min(timed(lambda: plain(16, 2))[1] for _ in range(3)) / 16
    say(f"seconds a sample of {o.shape[0]} rays: Scene.radiance {per_plain:.4f} (a call of 16); Scene.radiance(direct=\"mis\") {per_mis:.4f} "
        f"(a call of 16), {per_mis_1:.4f} (a call of 1); PathBatch(direct=\"mis\").run(50) {per_batch:.4f}: the new call takes "
        f"{per_mis / per_batch:.2f} of the batch's time a sample, {per_mis / per_plain:.2f} plain samples")
    for spp in (16, 64):
        a, t_plain = timed(lambda: plain(spp, 2)["radiance"])
        mm = max(1, int(round(t_plain / per_mis)))
        m, t_mis = timed(lambda: mis(mm, 5)["radiance"])
        mb = max(1, int(round(t_plain / per_batch)))
        b, t_batch = timed(lambda: batch_radiance(scene, o, d, time0, mb, 7))
        say(f"mean radiance of the reference {float(ref.mean()):.4f}; Scene.radiance at {spp} samples against both MIS forms at equal time:")
        say(f"  Scene.radiance                {spp:4d} samples  {t_plain:7.3f} s  RMSE {rmse(a):.4f}")
        say(f"  Scene.radiance(direct=\"mis\")  {mm:4d} samples  {t_mis:7.3f} s  RMSE {rmse(m):.4f}")
        say(f"  PathBatch(direct=\"mis\")       {mb:4d} samples  {t_batch:7.3f} s  RMSE {rmse(b):.4f}")
        for name, x in (("Scene.radiance", a), ("Scene.radiance(direct=\"mis\")", m), ("PathBatch(direct=\"mis\")", b)):
            err = (x - ref).abs().sum(dim=1)
            say(f"    {name:30s} mean {float(x.mean()):.4f}; median absolute error a ray {float(err.median()):.4f}, largest {float(err.max()):.2f}")
    # the kernel alone: its counts, its time by HIP events, its registers
    _, st = mis(16, 9, stats=True)
    say(f"one call of 16 samples with statistics: {st.rays} path searches, {st.shadow_rays} shadow rays cast, {st.shadow_reached} reached their "
        f"lamp; {st.seconds:.4f} s in the kernel (HIP events), {st.seconds / 16:.4f} s a sample; radiance_direct_kernel {st.kernel_vgprs} VGPRs, "
        f"{st.scratch_bytes} B scratch")
    _, sp = scene.radiance(o, d, time=time0, samples=16, max_depth=DEPTH, seed=9, stats=True)
    say(f"  plain Scene.radiance beside it: {sp.rays} path searches, {sp.seconds:.4f} s in the kernel, {sp.seconds / 16:.4f} s a sample; "
        f"radiance_kernel {sp.kernel_vgprs} VGPRs, {sp.scratch_bytes} B scratch")
    out = sys.argv[sys.argv.index("--output") + 1] if "--output" in sys.argv else os.path.join(ROOT, "profiles", "r24_radiance_direct.txt")
    with open(out, "w") as f:
        f.write("\n".join(_record) + "\n")


if __name__ == "__main__":
    main()
