"""Mesh builders shared by tests/test_triangles_host.py and tests/test_triangles_gpu.py (numpy only)."""
import numpy as np


def icosphere(levels, radius):
    """An icosahedron with its vertices on the sphere of ``radius`` about the origin, every face split in four ``levels`` times with
    the new vertices pushed out onto the sphere: (vertices (N, 3) float64, faces (20 * 4 ** levels, 3) int32), outward winding."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    verts = [radius * np.asarray(p, dtype=np.float64) / np.sqrt(1.0 + g * g) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid_of = {}

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid_of:
                m = verts[a] + verts[b]
                verts.append(radius * m / np.sqrt(m @ m))
                mid_of[key] = len(verts) - 1
            return mid_of[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.int32)


def lattice(n, size=1.0, y=0.0):
    """A flat n x n lattice of 2 n^2 triangles on the plane y: (vertices ((n + 1)^2, 3), faces (2 n^2, 3)).  Every cell is split
    along the same diagonal, so neighbours share whole edges and nothing else."""
    k = np.arange(n + 1, dtype=np.float64) * size
    x, z = np.meshgrid(k, k, indexing="ij")
    verts = np.stack([x.ravel(), np.full(x.size, y), z.ravel()], axis=-1)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]
    return verts, np.array(faces, dtype=np.int32)


def corners(q, u, v):
    """The three corners as the library computes them: Q, fl(Q + u), fl(Q + v)."""
    q, u, v = (np.asarray(a, dtype=np.float64) for a in (q, u, v))
    return np.stack([q, q + u, q + v])
