"""Moving instances: what the fourth kind of chain step costs the workloads that hold none -- c4, s8, c5, s13 on untouched kernels,
s14 on the affine units that learned the step -- and the first numbers for a scene that moves (the method and shape of
profiles/transform_measure.py).

  timeout -k 10 1100 python profiles/motion_measure.py --parent DIR          # the A/B and the demonstration scene, one call
  python profiles/motion_measure.py --run                                    # one run of every workload (a child of the above)

--parent DIR: a checkout of the parent commit, built.  The driver starts one process a run, the parent's tree and this one
alternately, --rounds runs each (default 5), each under its own time limit; a run of the parent is its own
profiles/transform_measure.py --run, a run of this tree renders the same five workloads and the demonstration scene:
  c4, s8, c5, s13, s14   as profiles/transform_measure.py states them
  x10    scene 7's room with its two boxes under static Transforms alone (RotateZ + Translate; RotateY + Scale + Translate), BVH world,
         800 x 800 x 300 spp, 3 frames after a warm-up, fast and strict: the five-wave instanced kernel (kind 10, 96 VGPRs) of the
         affine units, which scene 14 does not reach.  Both sides build it with this script (--tree names the package to load).
  demo   (this tree only) scene 14's room built through the Python API with the icosphere tumbling (a MovingTransform between two
         rotations 16 degrees apart, 60 units of travel), the slab sliding (a MovingTranslate of 120 units) and the fog drifting
         (the medium's boundary under a MovingTranslate of 80 units); shutter [0, 1]; 400 x 400 x 64 spp, strict build, 3 frames
After the runs the driver prints, per shared workload, both sides' min, median and max, whether this tree's median lies outside
the parent's range by more than its width, and whether both sides rendered one frame hash."""
import argparse
import os
import statistics
import subprocess
import sys

import transform_measure

HERE = os.path.dirname(os.path.abspath(__file__))
SHARED = "c4,s8,c5,s13,s14"
X10 = ("x10fast", "x10strict")


def cornell_room(s):
    red, white, green = s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.12, 0.45, 0.15))
    light = s.DiffuseLight((15.0, 15.0, 15.0))
    return white, [s.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green), s.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),
                   s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), light), s.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white),
                   s.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white), s.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)]


def x10_scene(rt):
    s = rt.Scene()
    white, items = cornell_room(s)
    items.append(s.Translate(s.RotateZ(s.MakeBox((0, 0, 0), (165, 330, 165), white), 8.0), (265, 0, 295)))
    items.append(s.Translate(s.Scale(s.RotateY(s.MakeBox((0, 0, 0), (165, 165, 165), white), -18.0), (1.0, 1.2, 0.9)), (130, 0, 65)))
    s.SetWorld(s.BvhNode(items))
    s.Camera((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 0.0, (0.0, 0.0, 0.0))
    s.Commit()
    return s


def demo_scene(rt, np):
    s = rt.Scene()
    white, items = cornell_room(s)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    from triangle_meshes import icosphere
    verts, faces = icosphere(2, 100.0)

    def turned(degrees, t):   # scene 14's matrix: scale (1.1, 1.6, 0.8), then a turn about Z, then a move
        a = np.radians(degrees)
        L = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.diag((1.1, 1.6, 0.8))
        return np.concatenate([L + 0.0, np.asarray(t, dtype=np.float64)[:, None]], axis=1)
    mesh = s.TriangleMesh(verts, faces, white, normals=verts / 100.0)
    items.append(s.MovingTransform(mesh, turned(17.0, (350.0, 175.0, 400.0)), turned(33.0, (410.0, 175.0, 400.0))))
    slab = s.MakeBox((0, 0, 0), (150, 40, 150), s.Metal((0.8, 0.85, 0.88), 0.0))
    items.append(s.MovingTranslate(s.RotateX(slab, -20.0), (60, 60, 250), (180, 60, 250)))
    items.append(s.Translate(s.Scale(s.Sphere((0, 0, 0), 1.0, s.Dielectric(1.5)), (90.0, 55.0, 70.0)), (170, 200, 120)))
    unit = s.MakeBox((0, 0, 0), (1, 1, 1), white)
    items.append(s.ConstantMedium(s.MovingTranslate(s.Scale(unit, (120.0, 200.0, 120.0)), (330, 330, 60), (250, 330, 60)), 0.01, (1.0, 1.0, 1.0)))
    s.SetWorld(s.BvhNode(items))
    s.Camera((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0, (0.0, 0.0, 0.0))
    s.Commit()
    return s


def run_all(only=None, tree=None):
    root = os.path.abspath(tree) if tree else os.path.dirname(HERE)
    sys.path.insert(0, root)
    import hashlib
    import numpy as np
    import raytracinginoneweekendincuda_amd as rt
    assert os.path.abspath(rt.__file__).startswith(root + os.sep), "the package of the tree that was asked for"

    def frames(name, scene, w, h, spp, variant):
        film = rt.Film(w, h)
        film.render(scene, 8, variant=variant)
        film.render(scene, spp, variant=variant)
        seconds = []
        for _ in range(3):
            st = film.render(scene, spp, variant=variant)
            seconds.append(st.seconds_seed + st.seconds_render)
        t = sum(seconds) / len(seconds)
        digest = hashlib.sha256(np.ascontiguousarray(film.download()).tobytes()).hexdigest()[:12]
        print(f"{name:9s} {w * h * spp / t * 1e-6:10.2f} Msamples/s {1e3 * t:11.3f} ms per step  {st.rays / (w * h * spp):.10f} rays per sample  "
              f"kind {st.kernel_kind}  {st.kernel_vgprs} VGPRs  frame {digest}", flush=True)

    for name in SHARED.split(","):
        if only is None or name in only:
            transform_measure.run_all([name])
    if only is None or "x10" in only:
        scene = x10_scene(rt)
        frames(X10[0], scene, 800, 800, 300, 1)
        frames(X10[1], scene, 800, 800, 300, 0)
    if only is None or "demo" in only:
        frames("demo", demo_scene(rt, np), 400, 400, 64, 0)


def drive(parent, rounds):
    sides = [("parent", [os.path.join(os.path.abspath(parent), "profiles", "transform_measure.py"), "--run"]),
             ("parent", [os.path.abspath(__file__), "--run", "--only", "x10", "--tree", os.path.abspath(parent)]),
             ("this", [os.path.abspath(__file__), "--run"])]
    rates, hashes = {}, {}
    for k in range(1, rounds + 1):
        for side, command in sides:
            env = dict(os.environ)
            env.pop("RTOW_LIB_PATH", None)   # every tree loads its own library
            done = subprocess.run(["timeout", "-k", "10", "280", sys.executable] + command, env=env, capture_output=True, text=True)
            for line in done.stdout.splitlines():
                name, rest = line.split(None, 1)
                print(f"{name:9s} {side:6s} {k}  {rest}", flush=True)
                rates.setdefault((name, side), []).append(float(rest.split()[0]))
                hashes.setdefault(name, set()).add(rest.split()[-1])
            if done.returncode != 0:
                print(done.stderr[-2000:], flush=True)
                sys.exit(f"{side} run {k} ended with status {done.returncode}: nothing more is started")
    print()
    for name in SHARED.split(",") + list(X10):
        p, t = rates[(name, "parent")], rates[(name, "this")]
        width, median = max(p) - min(p), statistics.median(t)
        below = median < min(p) - width
        print(f"{name:9s} parent min {min(p):9.2f} median {statistics.median(p):9.2f} max {max(p):9.2f} | this min {min(t):9.2f} median {median:9.2f} "
              f"max {max(t):9.2f} Msamples/s | this median / parent median {median / statistics.median(p):.4f} | below the parent's range by more "
              f"than its width: {'YES' if below else 'no'} | one frame hash on both sides: {'yes' if len(hashes[name]) == 1 else 'NO'}", flush=True)
    t = rates[("demo", "this")]
    print(f"{'demo':7s} this min {min(t):9.2f} median {statistics.median(t):9.2f} max {max(t):9.2f} Msamples/s | frame {sorted(hashes['demo'])}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--only", help="comma-separated workloads (default: all)")
    ap.add_argument("--tree", help="with --run: the tree whose package is loaded (default: this one)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.run:
        run_all(args.only.split(",") if args.only else None, args.tree)
    elif args.parent:
        drive(args.parent, args.rounds)
    else:
        ap.error("--run or --parent DIR")
