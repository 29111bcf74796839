"""Moving instances restated in numpy from Scene.moving_transform_keys (include/rtow.h rt_moving_transform), on top of
transform_restated.py: per ray of time tm the parameter s, the matrices L, t and the inverse Li by the cofactor formula, then the
local ray and the way back of the hit point and the normal with those per-ray matrices.  One np.float64 operation per stated
operation, every intermediate stored (as_stored)."""
import numpy as np

import transform_restated as tr
from transform_restated import as_stored


def pose(keys, tm):
    """(s, L, t, Li) for the ray times ``tm``: (N,), (N, 3, 3), (N, 3), (N, 3, 3)."""
    L0, t0, dL, dt, time0, dtime = keys
    tm = as_stored(tm)
    s = as_stored(as_stored(tm - time0) / dtime)
    s = as_stored(np.fmin(np.fmax(s, 0.0), 1.0))   # fmax drops a NaN: key 0
    L = np.empty((len(s), 3, 3))
    for r in range(3):
        for c in range(3):
            L[:, r, c] = as_stored(L0[r, c] + as_stored(s * dL[r, c]))
    t = np.stack([as_stored(t0[r] + as_stored(s * dt[r])) for r in range(3)], axis=-1)

    def cof(a, b, c, d):   # (a * b) - (c * d)
        return as_stored(as_stored(L[:, a[0], a[1]] * L[:, b[0], b[1]]) - as_stored(L[:, c[0], c[1]] * L[:, d[0], d[1]]))
    cf = [[cof((1, 1), (2, 2), (1, 2), (2, 1)), cof((1, 2), (2, 0), (1, 0), (2, 2)), cof((1, 0), (2, 1), (1, 1), (2, 0))],
          [cof((0, 2), (2, 1), (0, 1), (2, 2)), cof((0, 0), (2, 2), (0, 2), (2, 0)), cof((0, 1), (2, 0), (0, 0), (2, 1))],
          [cof((0, 1), (1, 2), (0, 2), (1, 1)), cof((0, 2), (1, 0), (0, 0), (1, 2)), cof((0, 0), (1, 1), (0, 1), (1, 0))]]
    det = as_stored(as_stored(as_stored(L[:, 0, 0] * cf[0][0]) + as_stored(L[:, 0, 1] * cf[0][1])) + as_stored(L[:, 0, 2] * cf[0][2]))
    Li = np.empty_like(L)
    for r in range(3):
        for c in range(3):
            Li[:, r, c] = as_stored(cf[c][r] / det)
    return s, as_stored(L), as_stored(t), as_stored(Li)


def rows_each(m, p):
    """M_k p_k per ray k: per row r, ((m[r][0] * p.x) + (m[r][1] * p.y)) + (m[r][2] * p.z)."""
    p = as_stored(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([as_stored(as_stored(as_stored(m[:, r, 0] * x) + as_stored(m[:, r, 1] * y)) + as_stored(m[:, r, 2] * z)) for r in range(3)], axis=-1)


def columns_each(m, n):
    return rows_each(np.ascontiguousarray(np.swapaxes(m, 1, 2)), n)


# A chain as in transform_restated.py with a fourth kind of step: ("moving", keys), keys = Scene.moving_transform_keys(handle).
def local_rays(chain, o, d, tm):
    o, d = as_stored(o).copy(), as_stored(d).copy()
    for step in chain:
        if step[0] == "moving":
            _, _, t, Li = pose(step[1], tm)
            o, d = rows_each(Li, as_stored(o - t)), rows_each(Li, d)
        else:
            o, d = tr.local_rays([step], o, d)
    return as_stored(o), as_stored(d)


def forward_points(chain, p, tm):
    p = as_stored(p).copy()
    for step in reversed(chain):
        if step[0] == "moving":
            _, L, t, _ = pose(step[1], tm)
            p = as_stored(rows_each(L, p) + t)
        else:
            p = tr.forward_points([step], p)
    return as_stored(p)


def forward_vectors(chain, v, tm):
    v = as_stored(v).copy()
    for step in reversed(chain):
        v = rows_each(pose(step[1], tm)[1], v) if step[0] == "moving" else tr.forward_vectors([step], v)
    return as_stored(v)


def forward_normals(chain, n, tm):
    n = as_stored(n).copy()
    for step in reversed(chain):
        if step[0] == "moving":
            m = columns_each(pose(step[1], tm)[3], n)
            k = as_stored(1.0 / np.sqrt(tr.length_sq(m)))
            n = as_stored(k[:, None] * m)
        else:
            n = tr.forward_normals([step], n)
    return as_stored(n)


def frozen_matrix(keys, tau):
    """The 3x4 [L(s) | t(s)] a ray of time ``tau`` sees: what Scene.Transform takes for the static twin."""
    _, L, t, _ = pose(keys, np.array([tau], dtype=np.float64))
    return np.concatenate([L[0], t[0][:, None]], axis=1)


def build_chain(scene, child, steps):
    """transform_restated.build_chain with ("moving", (matrix0, matrix1, time0, time1)) and ("moving_translate", (offset0, offset1,
    time0, time1)) steps as well; both come back as ("moving", the stored keys)."""
    handle, chain = child, []
    for kind, arg in reversed(steps):
        if kind == "moving":
            handle = scene.MovingTransform(handle, *arg)
            chain.append(("moving", scene.moving_transform_keys(handle)))
        elif kind == "moving_translate":
            handle = scene.MovingTranslate(handle, *arg)
            chain.append(("moving", scene.moving_transform_keys(handle)))
        else:
            handle, one = tr.build_chain(scene, handle, [(kind, arg)])
            chain.append(one[0])
    return handle, chain[::-1]
