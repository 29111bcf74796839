"""A frame with light samples restated from public calls (include/rtow.h rt_render_launch_direct has the definition): per round the
camera ray of every pixel still sampling, from the pixel's own stream through ``Rng.from_state``; one sample of
``Scene.radiance(direct="mis", samples=1)`` for it from the stream where the camera left it; the sums, the stopping rule through
``rt.adaptive_converged``, and ``sqrt((1 / N) * sum)``.  Every operation is one IEEE double operation in the kernel's order, so the
strict build's frame equals this one bit for bit.  Used by tests/test_film_direct_host.py and tests/test_film_direct_gpu.py."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt

ALL = ("radiance", "path_rays", "rng_state")


def camera_rays_from(scene, states, width, height, pixels=None):
    """tests/test_radiance_gpu.py::camera_rays from given streams: the next camera ray of pixel k = j * width + i, drawn from
    ``states[k]`` ({d, v0..v4}), and the stream after those draws.  ``pixels``: the k to do (all by default); the other rows come
    back as zeros and their states as given.  Returns (origins (N, 3), directions (N, 3), times (N,), states (N, 6) uint32)."""
    cam = scene.dump_camera()
    origin, llc, hor, ver, cam_u, cam_v = (cam[3 * k:3 * k + 3] for k in (1, 2, 3, 4, 5, 6))
    lens_radius, time0, time1 = cam[24], cam[25], cam[26]
    n = width * height
    o, d, tm, after = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.array(states, dtype=np.uint32).reshape(n, 6).copy()
    for k in (range(n) if pixels is None else pixels):
        j, i = divmod(int(k), width)
        rng = rt.Rng.from_state(after[k])
        u = np.float64(np.float32(i) + np.float32(rng.uniform())) / np.float64(width)   # int + float adds in fp32
        v = np.float64(np.float32(j) + np.float32(rng.uniform())) / np.float64(height)
        while True:
            a, b = np.float64(rng.uniform()), np.float64(rng.uniform())
            p = 2.0 * np.array([a, b, 0.0]) - np.array([1.0, 1.0, 0.0])
            if p[0] * p[0] + p[1] * p[1] + p[2] * p[2] < 1.0:
                break
        rd = lens_radius * p
        offset = rd[0] * cam_u + rd[1] * cam_v
        tm[k] = time0 + np.float64(rng.uniform()) * (time1 - time0)
        o[k] = origin + offset
        d[k] = (((llc + u * hor) + v * ver) - origin) - offset
        after[k] = rng.state()
    return o, d, tm, after


def seeded_states(seed, width, height, pixels=None):
    """The streams a film is seeded with: curand_init(seed, j * width + i, 0).  ``pixels``: the k to seed (all by default); the
    other rows stay zero."""
    states = np.zeros((width * height, 6), dtype=np.uint32)
    for k in (range(width * height) if pixels is None else pixels):
        states[int(k)] = rt.Rng(seed, int(k)).state()
    return states


class Frame:
    """The running state of a restated frame: per pixel k = j * width + i the stream, the colour sum, n, the sum of y^2 and the
    mark; the counters of every round since the last ``begin_launch``.  ``pixels``: restate these k alone -- a large frame is
    compared at a few of its pixels; the others are held as marked from the start, their n stays 0 and the counters leave them out."""

    def __init__(self, scene, width, height, seed, pixels=None):
        self.scene, self.width, self.height = scene, width, height
        n = width * height
        self.states = seeded_states(seed, width, height, pixels)
        self.col = np.zeros((n, 3))
        self.n = np.zeros(n, dtype=np.uint32)
        self.q = np.zeros(n)
        self.marked = np.zeros(n, dtype=bool)
        if pixels is not None:
            self.marked[:] = True
            self.marked[np.asarray(pixels, dtype=np.int64)] = False
        self.y2 = []           # per round: (pixels, y^2 of their samples)
        self.begin_launch()

    def begin_launch(self):
        self.rays = self.samples = self.shadow_rays = self.shadow_reached = 0
        self.longest_path = 0

    def launch(self, spp, depth, strategy=1, rule=None, direct=True, variant=0):
        """One launch of ``spp`` samples at the most (``rule``: the arguments of rt.adaptive_converged behind the sums, or None),
        with light samples or, ``direct=False``, as the plain render takes them (the same loop over rt_scene_radiance)."""
        self.begin_launch()
        live = np.flatnonzero(~self.marked)
        for _ in range(spp):
            if not len(live):
                break
            o, d, tm, self.states = camera_rays_from(self.scene, self.states, self.width, self.height, live)
            out, st = self.scene.radiance(np.ascontiguousarray(o[live]), np.ascontiguousarray(d[live]), times=np.ascontiguousarray(tm[live]),
                                          rng_state=np.ascontiguousarray(self.states[live]), samples=1, max_depth=depth, want=ALL, stats=True,
                                          variant=variant, direct="mis" if direct else None, strategy=strategy)
            acc = out["radiance"]
            self.states[live] = out["rng_state"]
            self.col[live] = self.col[live] + acc
            self.n[live] += 1
            y = (acc[:, 0] + acc[:, 1]) + acc[:, 2]
            self.q[live] = self.q[live] + y * y
            self.y2.append((live.copy(), y * y))
            self.rays += int(out["path_rays"].sum())
            self.longest_path = max(self.longest_path, int(out["path_rays"].max()))
            self.samples += len(live)
            if direct:
                self.shadow_rays += int(st.shadow_rays)
                self.shadow_reached += int(st.shadow_reached)
            if rule is not None:
                stops = np.array([rt.adaptive_converged(int(self.n[k]), self.col[k, 0], self.col[k, 1], self.col[k, 2], self.q[k], *rule)
                                  for k in live], dtype=bool)
                self.marked[live[stops]] = True
                live = live[~stops]
        return self

    def pixels(self):
        """sqrt((1 / N) * col) with every pixel's own N, (height, width, 3)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / self.n.astype(np.float64)
            return np.sqrt(inv[:, None] * self.col).reshape(self.height, self.width, 3)

    def counts(self):
        return self.n.reshape(self.height, self.width).copy()
