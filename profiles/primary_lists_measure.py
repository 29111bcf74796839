"""Sphere-list frames with the camera rays' candidate lists on (default) against RT_FLAG_NO_PRIMARY_LISTS, in one process.

    python profiles/primary_lists_measure.py [--frames 5]

1. The built-in scenes 0-11 as HittableList worlds that the sphere-list kernel renders (kind 16), 600 x 400, 50 spp.
2. 485 spheres as in C2 but every centre's y random (r13's list without a run), 600 x 400, 200 spp.
Per case: frames alternate off / on, kernel time by HIP events (rt_render_stats.seconds_render, rehearsal included), the median and
the spread of each side, and whether the two frames are equal bit for bit.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import raytracinginoneweekendincuda_amd as rt  # noqa: E402


def random_y_list():
    src = rt.builtin_scene(11, 1, 600, 400)
    _, boxes = src.dump_leaves()
    centres, radii = 0.5 * (boxes[:, 0::2] + boxes[:, 1::2]), 0.5 * (boxes[:, 1] - boxes[:, 0])
    rnd = np.random.default_rng(13)
    s = rt.Scene()
    items = []
    for k, (c, r) in enumerate(zip(centres, radii)):
        y = float(c[1]) if r > 10 else float(rnd.uniform(0.2, 3.0))
        mat = s.Dielectric(1.5) if k % 9 == 0 else (s.Metal((0.7, 0.6, 0.5), 0.1) if k % 4 == 0 else s.Lambertian((0.2 + 0.05 * (k % 12), 0.4, 0.6)))
        items.append(s.Sphere((float(c[0]), y, float(c[2])), float(r), mat))
    s.SetWorld(s.HittableList(items))
    s.Camera((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), 20.0, 600 / 400, 0.1, 10.0)
    s.Commit()
    return s


def measure(name, scene, w, h, spp, frames):
    times = {0: [], rt.FLAG_NO_PRIMARY_LISTS: []}
    out = {}
    kind = None
    for k in range(frames + 1):  # the first pair warms up
        for flags in (rt.FLAG_NO_PRIMARY_LISTS, 0):
            film = rt.Film(w, h)
            st = film.render(scene, spp, flags=flags)
            kind = st.kernel_kind
            if k:
                times[flags].append(st.seconds_render * 1e3)
            out[flags] = film.download().copy()
    on, off = np.array(times[0]), np.array(times[rt.FLAG_NO_PRIMARY_LISTS])
    lists = scene.primary_lists(w, h)
    lens = [len(l) for l in lists if l is not None]
    print("%-28s kind %3d  off %8.3f ms (%.3f-%.3f)  on %8.3f ms (%.3f-%.3f)  %+6.1f %%  frames equal: %s  lists: %d of %d tiles, mean %.2f" % (
        name, kind, np.median(off), off.min(), off.max(), np.median(on), on.min(), on.max(), 100.0 * (np.median(on) / np.median(off) - 1.0),
        np.array_equal(out[0].view(np.uint64), out[rt.FLAG_NO_PRIMARY_LISTS].view(np.uint64)), len(lens), len(lists), float(np.mean(lens)) if lens else 0.0), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    args = ap.parse_args()
    w, h = 600, 400
    for scene_id in range(12):
        try:
            s = rt.builtin_scene(scene_id, 1, w, h)
        except rt.RtowError:
            continue
        plan = s.plan_launch(rt.RenderParams(w, h, 50, 50, 1984, 8, 0, 1, 0, 0, 0, None, 0, 0, 0, 0, 0, 0))
        if plan["kernel_kind"] != 16:
            continue
        measure("scene %d, 50 spp" % scene_id, s, w, h, 50, args.frames)
    measure("485 spheres, random y, 200 spp", random_y_list(), w, h, 200, args.frames)


if __name__ == "__main__":
    main()
