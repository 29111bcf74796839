"""Ray queries against the feature pass on the benchmark frames: 1200 x 800 centre rays of C2 (list), C3 (bvh) and scene 9.

  timeout -k 10 300 python profiles/query_measure.py

Per frame: the feature pass at samples = 0 (the same search plus the camera's arithmetic; its kernel is the parent commit's,
profiles/r11_kernel_table.txt), the closest-hit query with every output, with t alone, and the occlusion query, alternating, five
rounds after a warm-up.  The query runs on torch tensors (rt_scene_intersect_device: no copies).  Both calls are synchronous, so
both are timed the same way, wall clock around the call (best of the rounds; a launch, the kernel, a stream synchronisation);
the query's own HIP-event time is printed beside it.  Strict build, as bench.py uses for these frames.  One process, one GPU."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

W, H, ROUNDS = 1200, 800, 5
CONFIGS = {"C2 (scene 11, list)": (11, 1), "C3 (scene 0, bvh)": (0, 0), "scene 9 (bvh)": (9, 0)}
ALL = ("t", "normal", "uv", "albedo", "leaf", "front_face", "material")


def centre_rays(scene):
    cam = scene.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(W) + 0.5) / W)[None, :, None]
    v = ((np.arange(H) + 0.5) / H)[:, None, None]
    d = (((llc + u * hor) + v * ver) - origin).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d), float(cam[25])


def clocked(call):
    t0 = time.perf_counter()
    result = call()
    return time.perf_counter() - t0, result


def main():
    for name, (scene_id, world) in CONFIGS.items():
        earth = None
        if scene_id == 9:
            with np.load(os.path.join(ROOT, "tests", "golden", "earthmap_stb.npz")) as g:
                earth = np.ascontiguousarray(g["bytes"])
        scene = rt.builtin_scene(scene_id, world, W, H, earth=earth)
        o, d, time0 = centre_rays(scene)
        dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        film = rt.Film(W, H)
        runs = {
            "feature pass": lambda: film.render_features(scene, samples=0, variant=0),
            "closest, all outputs": lambda: scene.intersect(dev_o, dev_d, time=time0, want=ALL, stats=True),
            "closest, t only": lambda: scene.intersect(dev_o, dev_d, time=time0, want=("t",), stats=True),
            "occlusion": lambda: scene.occluded(dev_o, dev_d, time=time0, stats=True),
        }
        for call in runs.values():   # warm-up: uploads, code objects, allocations
            call()
        torch.cuda.synchronize()
        wall = {k: [] for k in runs}
        event = {k: [] for k in runs}
        stats = {}
        for _ in range(ROUNDS):
            for k, call in runs.items():
                t, result = clocked(call)
                wall[k].append(t)
                if result is not None:
                    stats[k] = result[1]
                    event[k].append(result[1].seconds)
        # the same answer as the feature pass (strict build: bit for bit)
        out = scene.intersect(dev_o, dev_d, time=time0, want=("t", "normal", "albedo"))
        albedo, normal, depth = film.features()
        hit = torch.isfinite(out["t"]).cpu().numpy()
        assert np.array_equal(hit, depth.reshape(-1) > 0)
        assert np.array_equal(out["normal"].cpu().numpy().view(np.uint64), normal.reshape(-1, 3).view(np.uint64))
        assert np.array_equal(out["albedo"].cpu().numpy().view(np.uint64), albedo.reshape(-1, 3).view(np.uint64))
        rays = W * H
        # (the baseline is this build's feature pass: features_strict.o is the parent commit's byte for byte, profiles/r11_kernel_table.txt)
        base = min(wall["feature pass"])
        print(f"{name}: {rays} rays, {hit.mean():.3f} hit; baseline: this build's feature pass, whose object file is the parent's", flush=True)
        for k in runs:
            best = min(wall[k])
            line = f"  {k:22s} wall {1e3 * best:7.3f} ms = {rays / best * 1e-6:7.1f} Mrays/s ({best / base:.3f} of the feature pass)"
            if event[k]:
                st = stats[k]
                line += f"; kernel {1e3 * min(event[k]):7.3f} ms = {rays / min(event[k]) * 1e-6:7.1f} Mrays/s, {st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch"
            print(line, flush=True)


if __name__ == "__main__":
    main()
