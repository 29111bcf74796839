"""General affine instances restated in numpy from Scene.transform_matrices (include/rtow.h rt_transform): the local ray, the way
back of the hit point and of the normal, chains mixed with Translate / RotateY, and the light collector's rows.  One np.float64
operation per stated operation, every intermediate stored (as_stored), so nothing is contracted or kept wider on this side."""
import math

import numpy as np


def as_stored(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def rows(m, p):
    """M p for (N, 3) points: per row r, ((m[r][0] * p.x) + (m[r][1] * p.y)) + (m[r][2] * p.z)."""
    p = as_stored(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([as_stored(as_stored(as_stored(m[r, 0] * x) + as_stored(m[r, 1] * y)) + as_stored(m[r, 2] * z)) for r in range(3)], axis=-1)


def columns(m, n):
    """M^T n: per column c, ((m[0][c] * n.x) + (m[1][c] * n.y)) + (m[2][c] * n.z)."""
    return rows(np.ascontiguousarray(m.T), n)


# A chain is a list of steps, outermost first, as the instances wrap the child:
#   ("translate", offset)   ("rotate_y", degrees)   ("transform", (L, t, Li)) with the matrices of Scene.transform_matrices
def _sin_cos(degrees):
    radians = degrees * 3.1415926535897932385 / 180.0   # rt_rotate_y's conversion
    return np.float64(math.sin(radians)), np.float64(math.cos(radians))   # the C library's, as std::sin / std::cos


def local_rays(chain, o, d):
    """The ray the child's Hit is called with: every step's inverse, outermost first (R/Instance.h:46, :121-131, rtow.h Hit)."""
    o, d = as_stored(o).copy(), as_stored(d).copy()
    for kind, arg in chain:
        if kind == "translate":
            o = as_stored(o - np.asarray(arg, dtype=np.float64))
        elif kind == "rotate_y":
            st, ct = _sin_cos(arg)
            o, d = (np.stack([as_stored(as_stored(ct * v[:, 0]) - as_stored(st * v[:, 2])), v[:, 1],
                              as_stored(as_stored(st * v[:, 0]) + as_stored(ct * v[:, 2]))], axis=-1) for v in (o, d))
        else:
            L, t, Li = arg
            o, d = rows(Li, as_stored(o - t)), rows(Li, d)
    return as_stored(o), as_stored(d)


def forward_points(chain, p):
    """P of the hit record: every step's forward map, innermost first; a Transform's is (L P') + t."""
    p = as_stored(p).copy()
    for kind, arg in reversed(chain):
        if kind == "translate":
            p = as_stored(p + np.asarray(arg, dtype=np.float64))
        elif kind == "rotate_y":
            st, ct = _sin_cos(arg)
            p = np.stack([as_stored(as_stored(ct * p[:, 0]) + as_stored(st * p[:, 2])), p[:, 1],
                          as_stored(as_stored(-st * p[:, 0]) + as_stored(ct * p[:, 2]))], axis=-1)
        else:
            L, t, Li = arg
            p = as_stored(rows(L, p) + t)
    return as_stored(p)


def forward_vectors(chain, v):
    """u, v of a light row and a moving sphere's dc: the rotations and L, no offsets."""
    v = as_stored(v).copy()
    for kind, arg in reversed(chain):
        if kind == "rotate_y":
            st, ct = _sin_cos(arg)
            v = np.stack([as_stored(as_stored(ct * v[:, 0]) + as_stored(st * v[:, 2])), v[:, 1],
                          as_stored(as_stored(-st * v[:, 0]) + as_stored(ct * v[:, 2]))], axis=-1)
        elif kind == "transform":
            v = rows(arg[0], v)
    return as_stored(v)


def length_sq(n):
    return as_stored(as_stored(as_stored(n[:, 0] * n[:, 0]) + as_stored(n[:, 1] * n[:, 1])) + as_stored(n[:, 2] * n[:, 2]))


def forward_normals(chain, n):
    """Normal of the hit record: a RotateY turns it, a Transform takes it through Li^T and renormalises it, (1 / sqrt(|n|^2)) * n."""
    n = as_stored(n).copy()
    for kind, arg in reversed(chain):
        if kind == "rotate_y":
            st, ct = _sin_cos(arg)
            n = np.stack([as_stored(as_stored(ct * n[:, 0]) + as_stored(st * n[:, 2])), n[:, 1],
                          as_stored(as_stored(-st * n[:, 0]) + as_stored(ct * n[:, 2]))], axis=-1)
        elif kind == "transform":
            m = columns(arg[2], n)
            k = as_stored(1.0 / np.sqrt(length_sq(m)))
            n = as_stored(k[:, None] * m)
    return as_stored(n)


def build_chain(scene, child, steps):
    """Wraps ``child`` in the instances ``steps`` describe, outermost first -- ("translate", offset), ("rotate_y", degrees),
    ("transform", 3x4 matrix) -- and returns (handle, the chain with each matrix replaced by the stored (L, t, Li))."""
    handle, chain = child, []
    for kind, arg in reversed(steps):
        if kind == "translate":
            handle = scene.Translate(handle, arg)
            chain.append((kind, arg))
        elif kind == "rotate_y":
            handle = scene.RotateY(handle, arg)
            chain.append((kind, arg))
        else:
            handle = scene.Transform(handle, arg)
            chain.append((kind, scene.transform_matrices(handle)))
    return handle, chain[::-1]
