"""Triangle meshes: the first numbers for this path.

  timeout -k 10 300 python profiles/mesh_measure.py

1. Scene 12 (Cornell walls, a 320-triangle icosphere and a 20-triangle icosahedron as instanced groups with sub-BVHs) at
   400 x 400 x 64 spp, default against RT_FLAG_REFERENCE_TREE and against the general kernel, alternating, three rounds after a
   warm-up: Msamples/s and Mray/s from the render's own times (seeding + kernel, HIP events), best of the rounds.  Strict build.
2. Closest-hit and occlusion queries of 1200 x 800 rays against a 1280-triangle icosphere that is the BVH world itself (the
   library's tree over triangle leaves), on torch tensors (no copies): wall clock around the call and the query's HIP-event time.
3. The edge-leak count: rays aimed from outside at the shared edges and vertices of that closed icosphere -- every vertex, every
   edge midpoint and quarter point that faces the ray's origin.  Each triangle decides by its own rounded alpha and beta, so a ray
   may be rejected by both neighbours of an edge; it then passes between them and reports the far side of the mesh (or nothing).
   Counted, not asserted: the quad arithmetic promises no watertightness.
One process, one GPU."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402
from triangle_meshes import icosphere  # noqa: E402  (the tests' mesh builder)

ROUNDS = 3


def scene_12():
    w = h = 400
    spp = 64
    scene = rt.builtin_scene(12, 0, w, h)
    film = rt.Film(w, h)
    # (eight world leaves: the first two plan to the same kernel over the same tree; the third is the general kernel)
    runs = {"default": 0, "RT_FLAG_REFERENCE_TREE": rt.FLAG_REFERENCE_TREE,
            "... | RT_FLAG_FORCE_GENERAL": rt.FLAG_REFERENCE_TREE | rt.FLAG_FORCE_GENERAL}
    film.render(scene, 4, variant=0)   # warm-up: upload, code objects
    best = {}
    frames = {}
    for _ in range(ROUNDS):
        for name, flags in runs.items():
            st = film.render(scene, spp, variant=0, flags=flags)
            s = st.seconds_seed + st.seconds_render
            if name not in best or s < best[name][0]:
                best[name] = (s, int(st.rays), int(st.kernel_kind), int(st.kernel_vgprs))
            frames[name] = film.download()
    info = scene.info()
    print(f"scene 12, {w} x {h} x {spp} spp, strict build: {info['n_triangles']} triangles, {info['n_leaves']} world leaves, "
          f"{info['n_objects']} objects, {info['n_nodes']} threaded nodes", flush=True)
    for name, (s, rays, kind, vgprs) in best.items():
        print(f"  {name:24s} {1e3 * s:8.2f} ms  {w * h * spp / s * 1e-6:8.1f} Msamples/s  {rays / s * 1e-6:8.1f} Mray/s  "
              f"(kernel kind {kind}, {vgprs} VGPRs, {rays / (w * h * spp):.3f} rays per sample)", flush=True)
    same = all(np.array_equal(frames["default"].view(np.uint64), f.view(np.uint64)) for f in frames.values())
    print(f"  the three frames are {'equal bit for bit' if same else 'DIFFERENT'}", flush=True)


def clocked(call):
    t0 = time.perf_counter()
    result = call()
    return time.perf_counter() - t0, result


def icosphere_queries():
    w, h = 1200, 800
    radius, centre = 1.0, np.array([0.0713, -0.0319, -3.0117])
    verts, faces = icosphere(3, radius)
    s = rt.Scene()
    s.SetWorld(s.TriangleMesh(verts + centre, faces, s.Lambertian((0.5, 0.5, 0.5))))
    s.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, w / h, 0.0, 1.0)
    s.Commit()
    cam = s.dump_camera()
    origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(1, 5))
    u = ((np.arange(w) + 0.5) / w)[None, :, None]
    v = ((np.arange(h) + 0.5) / h)[:, None, None]
    d = np.ascontiguousarray((((llc + u * hor) + v * ver) - origin).reshape(-1, 3))
    o = np.ascontiguousarray(np.broadcast_to(origin, d.shape))
    dev_o, dev_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    runs = {"closest, all outputs": lambda: s.intersect(dev_o, dev_d, stats=True),
            "closest, t only": lambda: s.intersect(dev_o, dev_d, want=("t",), stats=True),
            "occlusion": lambda: s.occluded(dev_o, dev_d, stats=True)}
    for call in runs.values():
        call()
    torch.cuda.synchronize()
    wall, event = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(5):
        for k, call in runs.items():
            t, result = clocked(call)
            wall[k].append(t)
            event[k].append(result[1].seconds)
    hit = torch.isfinite(s.intersect(dev_o, dev_d, want=("t",))["t"]).float().mean().item()
    rays = w * h
    print(f"icosphere of {faces.shape[0]} triangles as the BVH world ({s.dump_fast_nodes()[0].shape[0]} nodes in the library's tree): "
          f"{rays} rays, {hit:.3f} hit", flush=True)
    for k in runs:
        print(f"  {k:22s} wall {1e3 * min(wall[k]):7.3f} ms = {rays / min(wall[k]) * 1e-6:7.1f} Mrays/s; kernel {1e3 * min(event[k]):7.3f} ms = "
              f"{rays / min(event[k]) * 1e-6:7.1f} Mrays/s", flush=True)
    return s, verts + centre, faces, centre


def edge_leaks(s, verts, faces, centre):
    edges = set()
    for a, b, c in faces:
        edges |= {(min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))}
    e = np.array(sorted(edges))
    p0, p1 = verts[e[:, 0]], verts[e[:, 1]]
    targets = np.concatenate([verts, 0.5 * (p0 + p1), 0.25 * p0 + 0.75 * p1, 0.75 * p0 + 0.25 * p1])
    total = leaks = missed = 0
    for origin in ((0.0, 0.0, 0.0), (2.3, 1.1, -1.2), (-1.9, -2.2, -3.9), (0.4, 2.8, -4.6)):
        origin = np.array(origin)
        d = targets - origin
        facing = np.einsum("ij,ij->i", targets - centre, -d) > 0.2 * np.linalg.norm(d, axis=1)   # well inside the silhouette
        o = np.ascontiguousarray(np.broadcast_to(origin, d.shape)[facing])
        t = s.intersect(o, np.ascontiguousarray(d[facing]), want=("t",))["t"]   # the target lies at t = 1
        total += t.size
        leaks += int(np.sum(~(np.abs(t - 1.0) <= 1e-6)))
        missed += int(np.sum(~np.isfinite(t)))
    print(f"edge leaks: {leaks} of {total} rays aimed at shared edges and vertices ({e.shape[0]} edges, {verts.shape[0]} vertices, four "
          f"origins) report no hit within 1e-6 of the target ({missed} of them no hit at all); strict build", flush=True)


if __name__ == "__main__":
    scene_12()
    edge_leaks(*icosphere_queries())
