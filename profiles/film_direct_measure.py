"""Frames with light samples, measured: what Film.render(direct="mis") costs a sample on scene 9 beside the route it replaces --
Scene.radiance(direct="mis") over the frame's camera rays -- and beside the plain Film.render, what it buys at equal wall time,
and what it does to the adaptive run README describes as failing.

  timeout -k 10 1100 python profiles/film_direct_measure.py [--output FILE]

Writes profiles/r25_film_direct.txt (or FILE): a header and every line it prints.  Scene 9, depth 50, strict build, one process,
one GPU.  Kernel times are HIP events (rt_render_stats.seconds_render, rt_radiance_direct_stats.seconds); every pair compared is
run alternately, three times each behind a warm-up, and the medians are compared."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402
from light_measure import centre_rays, scene9  # noqa: E402

DEPTH, SPP, ROUNDS = 50, 16, 3
HEADER = """Frames with light samples, measured (python profiles/film_direct_measure.py; one MI355X, one process, strict build).

Scene 9, depth 50.  "frame": Film.render(direct="mis"), film_direct_kernel, its time rt_render_stats.seconds_render (HIP events
around the kernel).  "route": what a caller had to do before -- Scene.radiance(direct="mis", samples=16) over one ray a pixel of the
same frame (torch tensors on the device, nothing copied), radiance_direct_kernel, its time rt_radiance_direct_stats.seconds (HIP
events around the kernel).  Each is warmed up once, then run three times alternately; medians are compared, and the allowance is the
spread (largest minus smallest) of the route's three runs.
"""
_record = []


def say(line=""):
    print(line, flush=True)
    _record.append(line)


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def frame_against_route(w, h, gate):
    scene = scene9(w, h)
    o, d, time0 = centre_rays(scene, w, h)
    film = rt.Film(w, h)
    plain_film = rt.Film(w, h)

    def frame():
        return film.render(scene, SPP, direct="mis", max_depth=DEPTH, seed=1984)

    def route():
        return scene.radiance(o, d, time=time0, samples=SPP, max_depth=DEPTH, seed=1984, direct="mis", stats=True)[1]

    def plain():
        return plain_film.render(scene, SPP, max_depth=DEPTH, seed=1984)

    for call in (frame, route, plain):
        call()
    torch.cuda.synchronize()
    t_frame, t_route, t_plain, w_frame, w_route = [], [], [], [], []
    for _ in range(ROUNDS):
        st, tw = wall(frame)
        t_frame.append(st.seconds_render)
        w_frame.append(tw)
        rs, tw = wall(route)
        t_route.append(rs.seconds)
        w_route.append(tw)
        t_plain.append(plain().seconds_render)
    ds = film.direct_stats()
    per = lambda ts: " ".join(f"{t / SPP:.5f}" for t in ts)
    mf, mr, mp = (statistics.median(t) / SPP for t in (t_frame, t_route, t_plain))
    spread = (max(t_route) - min(t_route)) / SPP
    say(f"{w} x {h}, {SPP} samples, seconds a sample of {w * h} pixels (kernel, HIP events):")
    say(f"  frame {per(t_frame)}  median {mf:.5f}   (wall {statistics.median(w_frame) / SPP:.5f})")
    say(f"  route {per(t_route)}  median {mr:.5f}   (wall {statistics.median(w_route) / SPP:.5f}); spread of its three runs {spread:.5f}")
    say(f"  plain Film.render {per(t_plain)}  median {mp:.5f}: the frame with light samples takes {mf / mp:.2f} times the plain frame's time a sample")
    say(f"  frame / route {mf / mr:.3f}; frame: {st.rays} path searches, {ds.shadow_rays} shadow rays cast, {ds.shadow_reached} reached their lamp; "
        f"route: {rs.rays} path searches, {rs.shadow_rays} shadow rays (other streams: the route's rays go through the pixel centres)")
    say(f"  film_direct_kernel: {st.kernel_vgprs} VGPRs, {ds.scratch_bytes} B scratch, {st.lds_bytes} B LDS, kernel kind {st.kernel_kind}; "
        f"radiance_direct_kernel: {rs.kernel_vgprs} VGPRs, {rs.scratch_bytes} B scratch")
    if gate:
        ok = mf <= mr + spread
        say(f"THE ONE REQUIREMENT ON TIME: the frame may not take longer than the route, within the route's own spread: "
            f"{mf:.5f} against {mr:.5f} + {spread:.5f} s a sample -- {'it holds' if ok else 'IT FAILS'}.")
    return scene, mf, mp


def linear(film):
    return film.download() ** 2   # the film holds sqrt(mean)


def errors(x, ref):
    return float(np.sqrt(np.mean((x - ref) ** 2))), float(np.median(np.abs(x - ref).sum(axis=-1)))


def main():
    _record.append(HEADER)
    scene, t_direct, t_plain = frame_against_route(400, 400, gate=True)
    say()
    frame_against_route(1600, 1600, gate=False)
    say()
    w = h = 400
    ref_film = rt.Film(w, h)
    _, t_ref = wall(lambda: ref_film.render(scene, 5000, max_depth=DEPTH, seed=7))
    ref = linear(ref_film)
    say(f"reference: the plain frame at 5000 samples a pixel from another seed ({t_ref:.1f} s), linear (pixels squared); mean {ref.mean():.4f}")
    for n_plain in (16, 64):
        # the direct frame's samples are sized by measured wall time: a first guess from the kernel times a sample, one frame of it
        # timed beside the plain frame, and the count scaled by what the two took (a plain sample is cheaper in a longer frame)
        a, b = rt.Film(w, h), rt.Film(w, h)
        _, ta = wall(lambda: a.render(scene, n_plain, max_depth=DEPTH, seed=1984))
        guess = max(1, round(n_plain * t_plain / t_direct))
        _, tg = wall(lambda: b.render(scene, guess, direct="mis", max_depth=DEPTH, seed=1984))
        n_direct = max(1, round(guess * ta / tg))
        _, tb = wall(lambda: b.render(scene, n_direct, direct="mis", max_depth=DEPTH, seed=1984))
        (ra, ma), (rb, mb) = errors(linear(a), ref), errors(linear(b), ref)
        say(f"equal wall time: plain {n_plain} samples {ta:.4f} s RMSE {ra:.4f} median absolute error a pixel {ma:.4f} | "
            f"direct {n_direct} samples {tb:.4f} s RMSE {rb:.4f} median absolute error a pixel {mb:.4f}")
    say()
    cap = 500
    say(f"the adaptive run README describes as failing: scene 9, {w} x {h}, min_samples 32, check_interval 32, at most {cap} samples a pixel; "
        "RMSE of the linear frame against the 5000-sample frame")
    for tau in (0.05, 0.02):
        for direct in (None, "mis"):
            film = rt.Film(w, h)
            film.set_adaptive(32, 32, tau)
            st, t = wall(lambda: film.render(scene, cap, direct=direct, max_depth=DEPTH, seed=1984))
            counts = film.sample_counts()
            r, m = errors(linear(film), ref)
            say(f"  tau {tau} {'direct=mis' if direct else 'plain     '}: {t:.3f} s, {counts.mean():.1f} samples a pixel ({float(np.mean(counts == 32)):.3f} of the pixels stop "
                f"at 32, {float(np.mean(counts == cap)):.3f} reach the cap), RMSE {r:.4f}, median absolute error a pixel {m:.4f}")
    out = os.path.join(ROOT, "profiles", "r25_film_direct.txt")
    if "--output" in sys.argv:
        out = sys.argv[sys.argv.index("--output") + 1]
    with open(out, "w") as f:
        f.write("\n".join(_record) + "\n")


if __name__ == "__main__":
    main()
