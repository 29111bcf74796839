"""The environment's first numbers: scene 15 as a frame, and the two sampling kernels on 960 000 points (the size of
profiles/r20_advance.txt: 1200 x 800 centre rays' first hits).

  timeout -k 10 300 python profiles/environment_measure.py

Scene 15 (the static random spheres under the computed sky, 1200 x 800, 100 spp, fast build as bench.py renders list worlds of
this kind) once after a warm-up frame of 1 spp; then, on the first hits of its centre rays, rt_scene_sample_environment_device with
every output and rt_scene_environment_pdf_device of the sampled directions, on torch tensors, five rounds after a warm-up, the
kernels' own HIP-event times (best of the rounds).  One process, one GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

W, H, SPP, ROUNDS = 1200, 800, 100, 5


def main():
    scene = rt.sky_demo_scene(1, W, H)
    env = scene.environment()
    print(f"scene 15: sky {env['image'].shape[1]} x {env['image'].shape[0]}, brightest texel {env['image'].max():.0f}, "
          f"distribution {env['has_distribution']}, flags {scene.flags():#x}")
    film = rt.Film(W, H)
    film.render(scene, 1, variant=1)
    st = film.render(scene, SPP, variant=1)
    frame = film.download()
    print(f"frame {W} x {H} x {SPP} spp, fast: kernel kind {st.kernel_kind}, {st.kernel_vgprs} VGPRs, {st.lds_bytes} B LDS, "
          f"{st.seconds_render * 1e3:.1f} ms, {st.rays / st.seconds_render / 1e9:.3f} Grays/s, mean pixel {frame.mean():.4f}")
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(W) + 0.5) / W)[None, :, None]
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    d = np.ascontiguousarray((((llc + u * hor) + v * ver) - origin).reshape(-1, 3))
    o = np.ascontiguousarray(np.broadcast_to(origin, d.shape))
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hit = scene.path_step(dev_o, dev_d, time=float(cam[25]), want=("status", "origin", "normal", "material", "rng_state"))
    print(f"{len(d)} points ({int((hit['status'] == 2).sum())} on scattering surfaces)")
    for variant, name in ((0, "strict"), (1, "fast")):
        best = {"sample": (1e9, None), "pdf": (1e9, None)}
        for k in range(ROUNDS + 1):
            smp, s1 = scene.sample_environment(hit["origin"], normals=hit["normal"], materials=hit["material"], rng_state=hit["rng_state"],
                                               variant=variant, stats=True)
            _, s2 = scene.environment_pdf(hit["origin"], smp["direction"], want=("pdf", "light"), variant=variant, stats=True)
            if k:   # (the first round warms up)
                best["sample"] = min(best["sample"], (s1.seconds, s1), key=lambda x: x[0])
                best["pdf"] = min(best["pdf"], (s2.seconds, s2), key=lambda x: x[0])
        for key, (sec, s) in best.items():
            print(f"environment {key:6s} {name:6s}: {sec * 1e3:7.3f} ms, {len(d) / sec / 1e9:6.3f} G points/s, {s.kernel_vgprs} VGPRs, "
                  f"{s.scratch_bytes} B scratch, valid {s.valid} of {s.points}")


if __name__ == "__main__":
    main()
