"""The hit record of a triangle with corner normals / texture coordinates, restated in numpy from include/rtow.h rt_triangle_attr:
one IEEE double operation per arithmetic sign, in the header's order (numpy fuses nothing), and the helpers the vertex-attribute
tests share: corner attributes for a mesh, rays aimed at its faces, the reference's ImageTexture lookup."""
import numpy as np

from query_helpers import dot3


def corner_attributes(tri, corner_values, corner_faces):
    """(hits, 3 corners, width): the values of the corners of triangle ``tri[k]`` -- ``corner_values[corner_faces[tri[k]]]``."""
    return np.asarray(corner_values, dtype=np.float64)[np.asarray(corner_faces)[tri]]


def shading_normal(alpha, beta, flat_normal, front, n):
    """``flat_normal``: the flat twin's record normal (the geometric unit normal set against the ray), ``front`` its front_face,
    ``n`` (hits, 3, 3) the corner normals.  Returns (the record's normal, where ns fell back to ng)."""
    gamma = (1.0 - alpha) - beta
    ng = np.where(front[:, None], flat_normal, -flat_normal)
    m = (gamma[:, None] * n[:, 0] + alpha[:, None] * n[:, 1]) + beta[:, None] * n[:, 2]
    lsq = m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2]
    with np.errstate(all="ignore"):
        ns = (1 / np.sqrt(lsq))[:, None] * m
        fallback = ~(np.isfinite(lsq) & (lsq > 0.0)) | (dot3(ns, ng) <= 0.0)
    ns = np.where(fallback[:, None], ng, ns)
    return np.where(front[:, None], ns, -ns), fallback


def texture_uv(alpha, beta, t):
    """``t`` (hits, 3, 2): the corners' texture coordinates.  Returns (hits, 2): U, V."""
    gamma = (1.0 - alpha) - beta
    return (gamma[:, None] * t[:, 0] + alpha[:, None] * t[:, 1]) + beta[:, None] * t[:, 2]


def as_stored(x):
    """A ray query stores normal and albedo as 0 + x: no negative zeros."""
    return 0.0 + x


def rays_at_faces(verts, faces, per_face, rng, distance, both_sides=False):
    """``per_face`` rays at random interior points of every face (barycentrics at least 0.02 from every edge), from ``distance``
    along the face's outward normal plus a random offset (``both_sides``: every other ray from behind).  Returns (origins,
    directions, the face each ray is aimed at)."""
    verts = np.asarray(verts, dtype=np.float64)
    a, b, c = (verts[faces[:, k]] for k in range(3))
    face = np.repeat(np.arange(len(faces)), per_face)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=face.size) * 0.94 + 0.02
    target = w[:, :1] * a[face] + w[:, 1:2] * b[face] + w[:, 2:] * c[face]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    side = np.where(both_sides & (np.arange(face.size) % 2 == 1), -1.0, 1.0)[:, None]
    origins = target + side * distance * n[face] + 0.3 * distance * rng.uniform(-1.0, 1.0, size=target.shape) * (1.0 - np.abs(n[face]))
    return np.ascontiguousarray(origins), np.ascontiguousarray(target - origins), face


def image_texel(image, u, v):
    """R/Texture.h:110-133 ImageTexture::Value: clamp u, v to [0, 1], flip v, truncate to a texel, clamp the index; the colour is
    the byte / 255."""
    h, w = image.shape[:2]
    u = np.clip(u, 0.0, 1.0)
    v = 1.0 - np.clip(v, 0.0, 1.0)
    i = np.minimum((u * w).astype(np.int64), w - 1)
    j = np.minimum((v * h).astype(np.int64), h - 1)
    return (1.0 / 255.0) * image[j, i].astype(np.float64)
