"""Adaptive sampling on the benchmark frames: what it costs when it stops nothing, and what it gains when it does.

  python profiles/adaptive_measure.py overhead   # the Adaptive<> instantiation with min_samples above the cap (no pixel stops:
                                                 # the frame is the plain one bit for bit, asserted) against the plain kernel,
                                                 # alternating, C2 / C3 / C4 at their benchmark sizes and C5 at 200 spp
  python profiles/adaptive_measure.py gain       # C2 at cap 500 and C5 at cap 5000, tau = 0.1 / 0.05 / 0.02 (min_samples 32, check
                                                 # every 32): frame time, mean samples per pixel, RMSE and share of pixels whose
                                                 # 8-bit PPM value is the plain frame's

Times are the kernels' (HIP events: seeding, rehearsal and render).  The builds are bench.py's: strict for C2, C3, C5, fast for C4."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import raytracinginoneweekendincuda_amd as rt  # noqa: E402

# name: scene, world kind, width, height, spp, variant
CONFIGS = {"c2": (11, 1, 1200, 800, 500, 0), "c3": (0, 0, 1200, 800, 500, 0), "c4": (7, 0, 800, 800, 1000, 1), "c5": (9, 0, 1600, 1600, 5000, 0)}
NEVER = 1 << 30  # a min_samples no pixel reaches


def scene_of(name):
    scene_id, world, w, h, _, _ = CONFIGS[name]
    earth = None
    if scene_id == 9:
        with np.load(os.path.join(ROOT, "tests", "golden", "earthmap_stb.npz")) as g:
            earth = np.ascontiguousarray(g["bytes"])
    return rt.builtin_scene(scene_id, world, w, h, earth=earth)


def render(scene, w, h, spp, variant, adaptive=None):
    film = rt.Film(w, h)
    if adaptive:
        film.set_adaptive(*adaptive)
    st = film.render(scene, spp, variant=variant)
    return film.download(), film.sample_counts(), st, st.seconds_seed + st.seconds_render


def overhead():
    for name in ("c2", "c3", "c4", "c5"):
        _, _, w, h, spp, variant = CONFIGS[name]
        spp = 200 if name == "c5" else spp
        scene = scene_of(name)
        render(scene, w, h, spp, variant)  # warm-up
        plain_t, adapt_t = [], []
        for _ in range(3):
            pf, _, pst, t = render(scene, w, h, spp, variant)
            plain_t.append(t)
            af, counts, ast, t = render(scene, w, h, spp, variant, (NEVER, 1, 0.05, 0.01))
            adapt_t.append(t)
            assert np.array_equal(pf.view(np.uint64), af.view(np.uint64)) and np.all(counts == spp) and ast.samples == pst.samples
            assert ast.kernel_kind == pst.kernel_kind + 512 and ast.rays == pst.rays
        ms = lambda ts: " ".join(f"{1e3 * t:.1f}" for t in ts)
        print(f"{name} {w}x{h}x{spp} {'fast' if variant else 'strict'}: plain kind {pst.kernel_kind} {pst.kernel_vgprs} VGPRs: {ms(plain_t)} ms | "
              f"adaptive kind {ast.kernel_kind} {ast.kernel_vgprs} VGPRs: {ms(adapt_t)} ms | mean ratio {np.mean(adapt_t) / np.mean(plain_t):.4f} "
              f"(frames bit-identical)", flush=True)


def gain():
    for name in ("c2", "c5"):
        _, _, w, h, cap, variant = CONFIGS[name]
        scene = scene_of(name)
        if name == "c2":
            render(scene, w, h, cap, variant)  # warm-up
        ref, _, st, t = render(scene, w, h, cap, variant)
        ppm = lambda f: (256.0 * np.clip(f, 0.0, 0.999)).astype(np.int64)
        print(f"{name} {w}x{h}, fixed {cap} spp: {1e3 * t:.1f} ms, {st.samples / t * 1e-6:.0f} Msamples/s", flush=True)
        for tau in (0.1, 0.05, 0.02):
            f, counts, ast, ta = render(scene, w, h, cap, variant, (32, 32, tau, 0.01))
            rmse = float(np.sqrt(np.mean((f - ref) ** 2)))
            same = float(np.mean(np.all(ppm(f) == ppm(ref), axis=-1)))
            print(f"{name} tau {tau}: {1e3 * ta:.1f} ms ({ta / t:.3f} of fixed), {counts.mean():.1f} samples per pixel ({counts.mean() / cap:.3f} of the cap; "
                  f"{float(np.mean(counts == cap)):.3f} of the pixels at the cap, {float(np.mean(counts == 32)):.3f} at 32), "
                  f"{ast.samples / ta * 1e-6:.0f} Msamples/s, RMSE {rmse:.5f}, 8-bit pixels equal {same:.4f}", flush=True)


if __name__ == "__main__":
    {"overhead": overhead, "gain": gain}[sys.argv[1] if len(sys.argv) > 1 else "overhead"]()
