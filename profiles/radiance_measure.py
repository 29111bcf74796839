"""Radiance queries against the render kernels on the benchmark frames: the 1200 x 800 centre rays of C2 (scene 11, list), C3
(scene 0, bvh) and scene 9, 16 samples each.  One GPU job, one frame per step, every step under its own time limit:

  timeout -k 10 400 python profiles/radiance_measure.py c2 && timeout -k 10 200 python profiles/radiance_measure.py c3 &&
  timeout -k 10 200 python profiles/radiance_measure.py scene9

Per frame, alternating, best of five rounds after a warm-up, strict build:
  radiance query   Scene.radiance at 16 samples, library-seeded, on torch tensors (rt_scene_radiance_device: no copies): the
                   kernel's HIP-event time and stats.rays / seconds
  general render   a 16-spp Film.render of the same frame with RT_FLAG_FORCE_GENERAL | RT_FLAG_REFERENCE_TREE |
                   RT_FLAG_NO_PIXEL_CLASSES | RT_FLAG_ROW_MAJOR_TILES: the general kernels (the parent commit's objects, byte for
                   byte) doing the same kind of work -- the reference's tree or list, one lane per pixel -- but persistent waves
                   over a tile queue with the tables staged in LDS, and camera rays with lens and time jitter
  default render   the same frame as the library renders it when left alone
The render's time is stats.seconds_render (HIP events around the render kernel), its rays stats.rays.
Then the lanes: the 16 samples once more as 16 one-sample calls chained through rng_state (the same paths), for the rays every
sample of every ray takes.  A wave of 64 consecutive rays is busy until its slowest lane is done.  In the flattened loop that is
max over lanes of (sum over samples); a loop over samples around a loop over bounces would take sum over samples of (max over
lanes).  Utilisation = rays traced / (64 x that), summed over the waves."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

W, H, SPP, ROUNDS = 1200, 800, 16, 5
CONFIGS = {"c2": ("C2 (scene 11, list)", 11, 1), "c3": ("C3 (scene 0, bvh)", 0, 0), "scene9": ("scene 9 (bvh)", 9, 0)}
GENERAL = rt.FLAG_FORCE_GENERAL | rt.FLAG_REFERENCE_TREE | rt.FLAG_NO_PIXEL_CLASSES | rt.FLAG_ROW_MAJOR_TILES


def centre_rays(scene):
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(W) + 0.5) / W)[None, :, None]
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    d = (((llc + u * hor) + v * ver) - origin).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d), float(cam[25])


def main(which):
    name, scene_id, world = CONFIGS[which]
    earth = None
    if scene_id == 9:
        with np.load(os.path.join(ROOT, "tests", "golden", "earthmap_stb.npz")) as g:
            earth = np.ascontiguousarray(g["bytes"])
    scene = rt.builtin_scene(scene_id, world, W, H, earth=earth)
    o, d, time0 = centre_rays(scene)
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    film = rt.Film(W, H)

    def query():
        _, st = scene.radiance(dev_o, dev_d, time=time0, samples=SPP, want=("radiance",), stats=True)
        return st.seconds, st.rays, f"{st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch"

    def render(flags):
        st = film.render(scene, SPP, variant=0, flags=flags)
        return st.seconds_render, st.rays, f"kernel kind {st.kernel_kind}, {st.kernel_vgprs} VGPRs, {st.lds_bytes} B LDS"

    runs = {"radiance query": query, "general render": lambda: render(GENERAL), "default render": lambda: render(0)}
    for call in runs.values():   # warm-up: uploads, code objects, allocations
        call()
    torch.cuda.synchronize()
    best = {}
    for _ in range(ROUNDS):
        for k, call in runs.items():
            seconds, rays, what = call()
            if k not in best or seconds < best[k][0]:
                best[k] = (seconds, rays, what)
    print(f"{name}: {W * H} rays x {SPP} samples", flush=True)
    for k, (seconds, rays, what) in best.items():
        print(f"  {k:15s} kernel {1e3 * seconds:9.3f} ms, {rays:10d} rays = {rays / seconds * 1e-6:7.1f} Mray/s; {what}", flush=True)
    per_ray = {k: seconds / rays for k, (seconds, rays, _) in best.items()}
    print(f"  time per ray: the query takes {per_ray['radiance query'] / per_ray['general render']:.2f} of the general render's, "
          f"{per_ray['radiance query'] / per_ray['default render']:.2f} of the default render's", flush=True)
    state = None
    per_sample = []
    for _ in range(SPP):
        out = scene.radiance(dev_o, dev_d, time=time0, samples=1, rng_state=state, want=("path_rays", "rng_state"))
        state = out["rng_state"]
        per_sample.append(out["path_rays"].cpu().numpy().astype(np.int64))
    rays = np.stack(per_sample, axis=1).reshape(-1, 64, SPP)   # wave, lane, sample (1200 x 800 is a whole number of waves)
    assert rays.sum() == best["radiance query"][1], "the chained calls trace the paths of the one call"
    flattened = rays.sum() / (64.0 * rays.sum(axis=2).max(axis=1).sum())
    nested = rays.sum() / (64.0 * rays.max(axis=1).sum())
    print(f"  lanes: rays per sample {rays.mean():.2f} (longest {rays.max()}), per ray {rays.sum(axis=2).mean():.1f} (longest {rays.sum(axis=2).max()}); "
          f"utilisation of the flattened loop {flattened:.3f}, of samples around bounces {nested:.3f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
