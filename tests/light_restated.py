"""The light sampling queries restated in numpy, operation by operation as include/rtow.h states them (rt_scene_sample_lights,
rt_scene_light_pdf): what the strict build must return to the bit.  numpy's elementwise operations are single IEEE-754 double
operations and nothing is fused, like the strict build.  Shared by tests/test_lights_host.py (closed forms) and
tests/test_lights_gpu.py (bit for bit against the kernels)."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt

PI = 3.1415926535897932385
QUAD, TRIANGLE, SPHERE, MSPHERE = 0, 1, 2, 3


def seeded_states(count, seed=1984, first_sequence=0):
    """(count, 6) uint32: curand_init(seed, k + first_sequence, 0) for k < count, through the library's host RNG."""
    return np.array([rt.Rng(seed, k + first_sequence).state() for k in range(count)], dtype=np.uint32).reshape(count, 6)


class Streams:
    """XORWOW streams as rows {d, v0..v4} (csrc/rng.h); ``uniform(mask)`` advances the rows of the mask by one draw."""

    def __init__(self, states):
        self.s = np.array(states, dtype=np.uint32).reshape(-1, 6).copy()

    def uniform(self, mask=None):
        s = self.s
        m = np.ones(len(s), dtype=bool) if mask is None else mask
        d, v0, v1, v2, v3, v4 = (s[m, k] for k in range(6))
        t = v0 ^ (v0 >> np.uint32(2))
        new4 = (v4 ^ (v4 << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
        d = d + np.uint32(362437)
        s[m, 0], s[m, 1], s[m, 2], s[m, 3], s[m, 4], s[m, 5] = d, v1, v2, v3, v4, new4
        x = (new4 + d).astype(np.float32) * np.float32(2.3283064e-10) + np.float32(2.3283064e-10) / np.float32(2.0)
        out = np.zeros(len(s), dtype=np.float64)
        out[m] = x.astype(np.float64)
        return out


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def over(a, t):  # R/Vec3.h:103-106: v / t is (1 / t) * v
    return (1.0 / t)[..., None] * a


def centres(L, idx, tm):
    c = L["a"][idx].copy()
    mv = L["kind"][idx] == MSPHERE
    if mv.any():
        frac = (tm[mv] - L["c"][idx][mv, 0]) / L["c"][idx][mv, 1]
        c[mv] = L["a"][idx][mv] + frac[:, None] * L["b"][idx][mv]
    return c


def usable(pdf):
    return (pdf > 0.0) & (pdf < np.inf)


def texture(emission, mat, u, v, p):
    """The material's texture as the kernels' material_texture evaluates a solid colour or a checker of two."""
    spec = emission[int(mat)]
    if spec[0] == "solid":
        return np.array(spec[1], dtype=np.float64)
    _, inv_scale, even, odd = spec
    n = int(np.floor(inv_scale * p[0])) + int(np.floor(inv_scale * p[1])) + int(np.floor(inv_scale * p[2]))
    return np.array(even if n % 2 == 0 else odd, dtype=np.float64)


def sample_lights(L, points, states, strategy=0, normals=None, materials=None, times=None, time=0.0, emission=None):
    """rt_scene_sample_lights on the rows ``L`` (Scene.lights()).  ``emission``: {material row: ("solid", rgb) or ("checker",
    inv_scale, even rgb, odd rgb)}, or None (then no "emitted" / "contribution").  Returns a dict of every output."""
    with np.errstate(all="ignore"):
        n = len(points)
        P = np.asarray(points, dtype=np.float64)
        tm = np.full(n, float(time)) if times is None else np.asarray(times, dtype=np.float64)
        st = Streams(states)
        out = {"direction": np.zeros((n, 3)), "distance": np.zeros(n), "light": np.full(n, -1, dtype=np.int32), "pdf": np.zeros(n),
               "emitted": np.zeros((n, 3)), "scatter_pdf": np.zeros(n), "contribution": np.zeros((n, 3))}
        n_lights = len(L["kind"])
        if n_lights:
            cdf = L["cdf"][:, strategy]
            xi = st.uniform()
            idx = np.searchsorted(cdf, xi, side="left")   # the first k with cdf[k] >= xi
            chance = cdf[idx] - np.where(idx > 0, cdf[np.maximum(idx, 1) - 1], 0.0)
            kind = L["kind"][idx]
            planar = kind <= TRIANGLE
            S = np.zeros((n, 3))
            U = np.zeros(n)
            V = np.zeros(n)
            valid = np.zeros(n, dtype=bool)
            C = centres(L, idx, tm)
            if planar.any():
                m = planar
                ua = st.uniform(m)
                ub = st.uniform(m)
                flip = m & (kind == TRIANGLE) & (ua + ub > 1.0)
                ua = np.where(flip, 1.0 - ua, ua)
                ub = np.where(flip, 1.0 - ub, ub)
                Sp = (L["a"][idx] + ua[:, None] * L["b"][idx]) + ub[:, None] * L["c"][idx]
                D = Sp - P
                d2 = dot(D, D)
                ln = np.sqrt(d2)
                ud = over(D, ln)
                c = np.abs(dot(L["n"][idx], ud))
                density = (d2 / (c * L["s"][idx])) * chance
                ok = m & (d2 > 0.0) & (c != 0.0) & usable(density)
                S[m], U[m], V[m] = Sp[m], ua[m], ub[m]
                out["direction"][ok], out["distance"][ok], out["pdf"][ok] = ud[ok], ln[ok], density[ok]
                valid |= ok
            if (~planar).any():
                m = ~planar
                todo = m.copy()
                px, py, s = np.zeros(n), np.zeros(n), np.zeros(n)
                while todo.any():   # the lens loop of the camera
                    da = st.uniform(todo)
                    db = st.uniform(todo)
                    x, y = 2.0 * da - 1.0, 2.0 * db - 1.0
                    ss = x * x + y * y
                    px[todo], py[todo], s[todo] = x[todo], y[todo], ss[todo]
                    todo &= ~((ss < 1.0) & (ss > 0.0))
                oc = C - P
                d2 = dot(oc, oc)
                r2 = L["s"][idx] * L["s"][idx]
                w = over(oc, np.sqrt(d2))
                cosmax = np.sqrt(1.0 - r2 / d2)
                omc = 1.0 - cosmax
                z = 1.0 - s * omc
                rho = np.sqrt(1.0 - z * z)
                q = np.sqrt(s)
                ex, ey = (rho * px) / q, (rho * py) / q
                ax, ay, az = np.abs(w[:, 0]), np.abs(w[:, 1]), np.abs(w[:, 2])
                zero = np.zeros(n)
                e1x = over(np.stack([w[:, 2], zero, -w[:, 0]], axis=-1), np.sqrt(w[:, 2] * w[:, 2] + w[:, 0] * w[:, 0]))
                e1y = over(np.stack([-w[:, 1], w[:, 0], zero], axis=-1), np.sqrt(w[:, 1] * w[:, 1] + w[:, 0] * w[:, 0]))
                e1z = over(np.stack([zero, -w[:, 2], w[:, 1]], axis=-1), np.sqrt(w[:, 2] * w[:, 2] + w[:, 1] * w[:, 1]))
                first = (ax >= ay) & (ax >= az)
                e1 = np.where(first[:, None], e1x, np.where((ay >= az)[:, None], e1y, e1z))
                e2 = cross(w, e1)
                g = (z[:, None] * w + ex[:, None] * e1) + ey[:, None] * e2
                ud = over(g, np.sqrt(dot(g, g)))
                po = P - C   # the renderer's sphere test for the ray (P, ud)
                qa, qb, qc = dot(ud, ud), dot(po, ud), dot(po, po) - r2
                disc = qb * qb - qa * qc
                ln = (-qb - np.sqrt(disc)) / qa
                density = chance / ((2.0 * PI) * omc)
                ok = m & (d2 > r2) & (omc != 0.0) & usable(density) & (disc > 0.0) & (ln > 0.0)
                S[ok] = (P + ln[:, None] * ud)[ok]
                out["rim"] = m & ~(z - cosmax >= 1e-12)   # samples on the cone's rim: the density call's hit test may miss them
                out["direction"][ok], out["distance"][ok], out["pdf"][ok] = ud[ok], ln[ok], density[ok]
                valid |= ok
            out["light"] = idx.astype(np.int32)
            out.setdefault("rim", np.zeros(n, dtype=bool))
            out["sample"] = S
            out["valid"] = valid
            if emission is not None:
                for k in np.nonzero(valid)[0]:
                    out["emitted"][k] = texture(emission, L["material"][idx[k]], U[k], V[k], S[k])
            if normals is not None and materials is not None:
                c = dot(np.asarray(normals, dtype=np.float64), out["direction"])
                lam = np.where(c > 0.0, (2.0 * ((c * c) * c)) / PI, 0.0)
                mats = np.asarray(materials)
                sp = np.where(mats == 0, lam, np.where(mats == 4, 1.0 / (4.0 * PI), 0.0))
                sp = np.where(valid, sp, 0.0)
                out["scatter_pdf"] = sp
                wgt = sp / np.where(valid, out["pdf"], 1.0)
                out["contribution"] = np.where((sp != 0.0)[:, None], wgt[:, None] * out["emitted"], 0.0)
        out["rng_state"] = st.s
        return out


def light_pdf(L, origins, directions, strategy=0, times=None, time=0.0):
    """rt_scene_light_pdf on the rows ``L``: (pdf, nearest light)."""
    with np.errstate(all="ignore"):
        o = np.asarray(origins, dtype=np.float64)
        d = np.asarray(directions, dtype=np.float64)
        n = len(o)
        tm = np.full(n, float(time)) if times is None else np.asarray(times, dtype=np.float64)
        dd = dot(d, d)
        total = np.zeros(n)
        nearest = np.full(n, np.inf)
        light = np.full(n, -1, dtype=np.int32)
        before = 0.0
        for i in range(len(L["kind"])):
            upto = L["cdf"][i, strategy]
            chance = upto - before
            before = upto
            density = np.zeros(n)
            t = np.zeros(n)
            if L["kind"][i] <= TRIANGLE:
                nn, Q, U, V = L["n"][i][None], L["a"][i][None], L["b"][i][None], L["c"][i][None]
                denom = dot(nn, d)
                t = dot(nn, Q - o) / denom
                ph = (o + t[:, None] * d) - Q
                m = cross(U, V)
                mm = dot(m, m)
                alpha, beta = dot(m, cross(ph, V)) / mm, dot(m, cross(U, ph)) / mm
                below = (alpha + beta <= 1.0) if L["kind"][i] == TRIANGLE else ((alpha <= 1.0) & (beta <= 1.0))
                inside = (denom != 0.0) & (t > 0.0) & (0.0 <= alpha) & (0.0 <= beta) & below
                density = np.where(inside, (((t * t) * dd) / ((np.abs(denom) / np.sqrt(dd)) * L["s"][i])) * chance, 0.0)
            else:
                idx = np.full(n, i)
                oc = centres(L, idx, tm) - o
                d2 = dot(oc, oc)
                r2 = L["s"][i] * L["s"][i]
                b = dot(oc, d)
                disc = b * b - dd * (d2 - r2)
                omc = 1.0 - np.sqrt(1.0 - r2 / d2)
                hit = (d2 > r2) & (b > 0.0) & (disc >= 0.0)
                density = np.where(hit & (omc != 0.0), chance / ((2.0 * PI) * omc), 0.0)
                t = (b - np.sqrt(disc)) / dd
            ok = usable(density)
            total = np.where(ok, total + density, total)
            closer = ok & (t < nearest)
            nearest = np.where(closer, t, nearest)
            light = np.where(closer, i, light).astype(np.int32)
        return total, light
