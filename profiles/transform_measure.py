"""General affine instances: what the third kind of chain step costs the workloads that hold no Transform, and the first numbers
for scene 14 (the method of profiles/r16_triangle_ab.txt and profiles/vertex_attr_measure.py).

  timeout -k 10 900 python profiles/transform_measure.py --parent DIR        # the A/B and scene 14, one call
  python profiles/transform_measure.py --run                                 # one run of every workload (a child of the above)

--parent DIR: a checkout of the parent commit, built (its package and its librtow_hip.so).  The driver starts one process a run,
the parent's tree and this one alternately, --rounds runs each (default 5); a run of the parent is its own
profiles/vertex_attr_measure.py --run --only c4,s8,c5,s13, a run of this tree renders the same four and scene 14 with this
tree's package and prints a line each:
  c4     scene 7, BVH world, 800 x 800 x 1000 spp, fast build, 3 frames after a warm-up   (bench.py --workload c4)
  s8     scene 8, BVH world, 800 x 800 x 200 spp, strict build, 2 frames
  c5     scene 9, BVH world, 1600 x 1600 x 100 spp, strict build, 1 frame                (bench.py --workload c5 at 100 spp)
  s13    scene 13, BVH world, 400 x 400 x 64 spp, strict build, 3 frames
  s14    (this tree only) scene 14 -- scene 7's room with four general affine instances -- as s13
Frames are timed as bench.py times them: seeding + render kernel from the render's own HIP events, mean of the frames after the
warm-up.  "frame" is the first 12 hex digits of the sha256 of the downloaded frame.  After the runs the driver prints, per
workload, both sides' min, median and max and whether this tree's median lies outside the parent's range by more than its width."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHARED = "c4,s8,c5,s13"


def run_all(only=None):
    root = os.path.dirname(HERE)
    sys.path.insert(0, root)
    import numpy as np
    import raytracinginoneweekendincuda_amd as rt

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

    runs = {"c4": lambda: frames("c4", 7, 800, 800, 1000, 1, 3), "s8": lambda: frames("s8", 8, 800, 800, 200, 0, 2),
            "c5": lambda: frames("c5", 9, 1600, 1600, 100, 0, 1), "s13": lambda: frames("s13", 13, 400, 400, 64, 0, 3),
            "s14": lambda: frames("s14", 14, 400, 400, 64, 0, 3)}
    for name, run in runs.items():
        if only is None or name in only:
            run()


def drive(parent, rounds):
    sides = [("parent", [os.path.join(os.path.abspath(parent), "profiles", "vertex_attr_measure.py"), "--run", "--only", SHARED]),
             ("this", [os.path.abspath(__file__), "--run"])]
    rates, hashes = {}, {}
    for k in range(1, rounds + 1):
        for side, command in sides:
            env = dict(os.environ)
            env.pop("RTOW_LIB_PATH", None)   # every tree loads its own library
            done = subprocess.run([sys.executable] + command, env=env, capture_output=True, text=True, timeout=280)
            for line in done.stdout.splitlines():
                name, rest = line.split(None, 1)
                print(f"{name:7s} {side:6s} {k}  {rest}", flush=True)
                rates.setdefault((name, side), []).append(float(rest.split()[0]))
                hashes.setdefault(name, set()).add(rest.split()[-1])
            if done.returncode != 0:
                print(done.stderr[-2000:], flush=True)
                sys.exit(f"{side} run {k} ended with status {done.returncode}: nothing more is started")
    print()
    for name in SHARED.split(","):
        p, t = rates[(name, "parent")], rates[(name, "this")]
        width, median = max(p) - min(p), statistics.median(t)
        outside = median < min(p) - width or median > max(p) + width
        print(f"{name:7s} parent min {min(p):9.2f} median {statistics.median(p):9.2f} max {max(p):9.2f} | this min {min(t):9.2f} median {median:9.2f} "
              f"max {max(t):9.2f} Msamples/s | this median / parent median {median / statistics.median(p):.4f} | outside the parent's range by more "
              f"than its width: {'YES' if outside else 'no'} | one frame hash on both sides: {'yes' if len(hashes[name]) == 1 else 'NO'}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--only", help="comma-separated workloads (default: all)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.run:
        run_all(args.only.split(",") if args.only else None)
    elif args.parent:
        drive(args.parent, args.rounds)
    else:
        ap.error("--run or --parent DIR")
