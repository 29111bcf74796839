"""Corner normals and texture coordinates: what the hit record's new block costs the workloads that have no attributed triangle,
and the first numbers for the ones that have (the method of profiles/r16_triangle_ab.txt).

  timeout -k 10 900 python profiles/vertex_attr_measure.py --parent DIR        # the A/B and scene 13, one call
  python profiles/vertex_attr_measure.py --run                                 # one run of every workload (a child of the above)
  ... --only c4,c5 --rounds 5 --other NAME=LIBRARY                             # some workloads, more rounds, a third side

--parent DIR: a checkout of the parent commit, built (its package and its librtow_hip.so).  The driver starts one process a run,
the parent's tree and this one alternately, three runs each; a run renders every workload with the package of its own tree and
prints a line each:
  c4     scene 7, BVH world, 800 x 800 x 1000 spp, fast build, 3 frames after a warm-up   (bench.py --workload c4)
  s8     scene 8, BVH world, 800 x 800 x 200 spp, strict build, 2 frames
  c5     scene 9, BVH world, 1600 x 1600 x 100 spp, strict build, 1 frame                (bench.py --workload c5 at 100 spp)
  s12    scene 12, BVH world, 400 x 400 x 64 spp, strict build, 3 frames
  s7list / s7bvh   radiance queries along the 1200 x 800 centre rays of scene 7, 16 samples a ray, strict build, torch tensors,
         best of three (the kernel's HIP-event time)
  s13    (this tree only) scene 13 -- scene 12 with corner normals on both meshes -- as s12
Frames are timed as bench.py times them: seeding + render kernel from the render's own HIP events, mean of the frames after the
warm-up.  "frame" is the first 12 hex digits of the sha256 of the downloaded frame (of the radiance array for the queries)."""
import argparse
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROUNDS = 3


def run_all(only=None):
    root = os.path.dirname(HERE)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import torch
    import raytracinginoneweekendincuda_amd as rt
    from query_helpers import centre_rays

    earth = np.load(os.path.join(root, "tests", "golden", "earthmap_stb.npz"))["bytes"]
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]

    def frames(name, scene_id, w, h, spp, variant, steps):
        scene = rt.builtin_scene(scene_id, 0, w, h, earth=earth if scene_id == 9 else None)
        film = rt.Film(w, h)
        film.render(scene, min(spp, 8), variant=variant)   # warm-up: upload, code objects
        if steps > 1:
            film.render(scene, spp, variant=variant)
        seconds = []
        for _ in range(steps):
            st = film.render(scene, spp, variant=variant)
            seconds.append(st.seconds_seed + st.seconds_render)
        s = sum(seconds) / len(seconds)
        print(f"{name:7s} {w * h * spp / s * 1e-6:10.2f} Msamples/s {1e3 * s:11.3f} ms per step  {st.rays / (w * h * spp):.10f} rays per sample  "
              f"kind {st.kernel_kind}  {st.kernel_vgprs} VGPRs  frame {digest(film.download())}", flush=True)

    def radiance(name, world):
        w, h = 1200, 800
        scene = rt.builtin_scene(7, world, w, h)
        o, d, _, _ = centre_rays(scene, w, h)
        dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        best = None
        for _ in range(1 + ROUNDS):
            out, st = scene.radiance(dev_o, dev_d, samples=16, variant=0, want=("radiance",), stats=True)
            torch.cuda.synchronize()
            best = st.seconds if best is None else min(best, st.seconds)
        print(f"{name:7s} radiance {1e3 * best:9.3f} ms ({st.rays / best * 1e-6:9.1f} Mray/s, {st.kernel_vgprs} VGPRs, {st.scratch_bytes} B scratch)  "
              f"frame {digest(out['radiance'].cpu().numpy())}", flush=True)

    runs = {"c4": lambda: frames("c4", 7, 800, 800, 1000, 1, 3), "s8": lambda: frames("s8", 8, 800, 800, 200, 0, 2),
            "c5": lambda: frames("c5", 9, 1600, 1600, 100, 0, 1), "s12": lambda: frames("s12", 12, 400, 400, 64, 0, 3),
            "s7list": lambda: radiance("s7list", 1), "s7bvh": lambda: radiance("s7bvh", 0)}
    if "n_attributed_triangles" in rt.builtin_scene(12, 0, 40, 40).info():
        runs["s13"] = lambda: frames("s13", 13, 400, 400, 64, 0, 3)
    for name, run in runs.items():
        if only is None or name in only:
            run()


def drive(parent, only, rounds, other):
    """``other``: NAME=LIBRARY, a third side -- this tree's package over another build of its library (a form of the block under trial)."""
    sides = [("parent", os.path.join(os.path.abspath(parent), "profiles", "vertex_attr_measure.py"), None), ("this", os.path.abspath(__file__), None)]
    if other:
        sides.append((other.split("=")[0], os.path.abspath(__file__), os.path.abspath(other.split("=")[1])))
    for k in range(1, rounds + 1):
        for side, script, library in sides:
            env = dict(os.environ)
            env.pop("RTOW_LIB_PATH", None)   # every tree loads its own library
            if library:
                env["RTOW_LIB_PATH"] = library
            done = subprocess.run([sys.executable, script, "--run"] + (["--only", only] if only else []), env=env, capture_output=True, text=True,
                                  timeout=280)
            for line in done.stdout.splitlines():
                name, rest = line.split(None, 1)
                print(f"{name:7s} {side:6s} {k}  {rest}", flush=True)
            if done.returncode != 0:
                print(done.stderr[-2000:], flush=True)
                sys.exit(f"{side} run {k} ended with status {done.returncode}: nothing more is started")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--only", help="comma-separated workloads (default: all)")
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--other", metavar="NAME=LIBRARY")
    args = ap.parse_args()
    if args.run:
        run_all(args.only.split(",") if args.only else None)
    elif args.parent:
        drive(args.parent, args.only, args.rounds, args.other)
    else:
        ap.error("--run or --parent DIR")
