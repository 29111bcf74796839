"""The worlds of tests/golden/reference_hits.npz, each one callback for the library, the oracle and the reference
(rt.Scene / conftest.OracleScene / reference_scene.RefScene), and what the generator and the tests need to know of their shapes.

  mixed     query_helpers.mixed_world: every primitive, texture and material kind, two movers, no media
  cornell   a Cornell-style room with two Translate(RotateY(box)) instances, one of them the boundary of a ConstantMedium, and a
            medium with a sphere boundary around a glass sphere (the nesting of scene 9, small)
  nested    a BvhNode of eight spheres inside a HittableList under a Translate, beside a span-1 BvhNode (its leaf is tested
            twice, R/BvhNode.h:63-67) and a Quad whose plane contains the origin (mD == 0)

World kind 0 is the BvhNode world, 1 the HittableList world."""
import numpy as np

from query_helpers import mixed_world

W, H, SPP, SEED = 24, 16, 4, 1984
WORLDS = ("mixed", "cornell", "nested")
KINDS = (0, 1)
HITTABLES = ("Sphere", "MovingSphere", "Quad", "Translate", "RotateY", "MakeBox", "HittableList", "BvhNode", "ConstantMedium")


class Recorder:
    """A view of a scene that passes every call on and keeps the handle of every Hittable made, in the order of construction."""

    def __init__(self, scene):
        self.scene, self.hittables = scene, []

    def __getattr__(self, name):
        fn = getattr(self.scene, name)
        if name not in HITTABLES:
            return fn

        def made(*a, **kw):
            handle = fn(*a, **kw)
            self.hittables.append(handle)
            return handle
        return made


def cornell_world(s, Rng, world_kind, aspect):
    white, red, green = s.Lambertian((0.73, 0.73, 0.73)), s.Lambertian((0.65, 0.05, 0.05)), s.Lambertian((0.12, 0.45, 0.15))
    marble = s.Lambertian(s.NoiseTexture(2.0, Rng(1984, 0)))
    glass = s.Dielectric(1.5)
    items = [s.Quad((4, 0, 0), (0, 4, 0), (0, 0, 4), green), s.Quad((0, 0, 0), (0, 4, 0), (0, 0, 4), red),
             s.Quad((0, 0, 0), (4, 0, 0), (0, 0, 4), white), s.Quad((0, 0, 4), (4, 0, 0), (0, 4, 0), marble),
             s.Quad((1.5, 3.75, 1.5), (1, 0, 0), (0, 0, 1), s.DiffuseLight((15.0, 15.0, 15.0))),
             s.Translate(s.RotateY(s.MakeBox(*CORNELL_BOXES[0][:2], s.Metal((0.8, 0.85, 0.88), 0.6)), CORNELL_BOXES[0][2]), CORNELL_BOXES[0][3]),
             s.ConstantMedium(s.Translate(s.RotateY(s.MakeBox(*CORNELL_BOXES[1][:2], white), CORNELL_BOXES[1][2]), CORNELL_BOXES[1][3]),
                              3.0, (0.9, 0.9, 0.9)),
             s.ConstantMedium(s.Sphere(CORNELL_FOG[0], CORNELL_FOG[1], glass), 2.5, (0.2, 0.4, 0.9)),
             s.Sphere(CORNELL_GLASS[0], CORNELL_GLASS[1], glass)]
    s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
    s.Camera((2.0, 2.0, -5.5), (2.0, 2.0, 0.0), (0, 1, 0), 40.0, aspect, 0.0, 10.0, 0.0, 0.0, (0.05, 0.05, 0.1))
    s.Commit()
    return s


# MakeBox corners, RotateY degrees, Translate offset: Translate(RotateY(MakeBox(lo, hi), degrees), offset)
CORNELL_BOXES = (((0.0, 0.0, 0.0), (1.2, 2.4, 1.2), 15.0, (1.9, 0.0, 2.1)), ((0.0, 0.0, 0.0), (1.2, 1.2, 1.2), -18.0, (0.9, 0.0, 0.5)))
CORNELL_FOG = ((3.0, 0.9, 1.0), 0.7)      # the sphere boundary of the second medium
CORNELL_GLASS = ((3.0, 0.9, 1.0), 0.3)    # the glass sphere inside it

NESTED_OFFSET = (0.0, -0.5, 1.5)
NESTED_SPHERES = tuple(((-2.4 + 1.6 * (k % 4), -0.8 + 1.6 * (k // 4), 0.3 * (k % 3)), 0.7 + 0.05 * (k % 2)) for k in range(8))
NESTED_SINGLE = ((0.25, 0.9, -1.0), 1.25)


def nested_world(s, Rng, world_kind, aspect):
    glass = s.Dielectric(1.5)
    materials = [s.Lambertian((0.7, 0.3, 0.2)), s.Metal((0.8, 0.8, 0.7), 0.5), glass, s.DiffuseLight((2.0, 2.0, 1.5)), s.Isotropic((0.3, 0.8, 0.4)),
                 s.Lambertian(s.CheckerTexture(0.4, s.SolidColor((0.1, 0.1, 0.1)), s.SolidColor((0.9, 0.9, 0.2)))), s.Metal((0.9, 0.5, 0.5), 0.0), glass]
    eight = [s.Sphere(c, r, materials[k]) for k, (c, r) in enumerate(NESTED_SPHERES)]
    moved = s.Translate(s.HittableList([s.BvhNode(eight)]), NESTED_OFFSET)
    single = s.BvhNode([s.Sphere(NESTED_SINGLE[0], NESTED_SINGLE[1], glass)])
    quad = s.Quad(*NESTED_QUAD, s.Lambertian((0.4, 0.5, 0.7)))
    items = [moved, single, quad]
    s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
    s.Camera((0.5, 1.5, 6.0), (0.0, 0.0, 0.0), (0, 1, 0), 50.0, aspect, 0.05, 6.0, 0.0, 1.0, (0.6, 0.7, 0.9))
    s.Commit()
    return s


NESTED_QUAD = ((-3.0, -2.0, -2.0), (6.0, 0.0, 0.0), (0.0, 4.0, 4.0))   # the plane y == z


def build(name, s, Rng, world_kind):
    return {"mixed": mixed_world, "cornell": cornell_world, "nested": nested_world}[name](s, Rng, world_kind, W / H)


# ---- the shapes, for the generator's assertions ----
def containers(name):
    """What a ray can start inside of: (label, kind, parameters), kind "sphere" (centre, radius) or "box" (lo, hi, degrees, offset)."""
    if name == "mixed":
        return [("glass sphere", "sphere", ((0.0, 0.0, -1.0), 0.5))]
    if name == "cornell":
        return [("metal box", "box", CORNELL_BOXES[0]), ("medium box", "box", CORNELL_BOXES[1]), ("medium sphere", "sphere", CORNELL_FOG),
                ("glass sphere", "sphere", CORNELL_GLASS)]
    moved = tuple(a + b for a, b in zip(NESTED_SPHERES[2][0], NESTED_OFFSET))
    return [("glass sphere", "sphere", (moved, NESTED_SPHERES[2][1])), ("span-1 glass sphere", "sphere", NESTED_SINGLE)]


MEDIA = {"mixed": (), "cornell": ("medium box", "medium sphere"), "nested": ()}


def quads(name):
    """(q, u, v) of the world's free-standing quads, for rays parallel to their planes."""
    if name == "mixed":
        return [((-2.5, -0.5, -2.5), (5, 0, 0), (0, 2.5, 0)), ((-2.4, -0.5, -2.4), (0, 0, 2.5), (0, 1.5, 0.3)), ((2.0, -0.5, 0.2), (0.3, 0, -2.4), (0, 1.2, 0))]
    if name == "cornell":
        return [((4, 0, 0), (0, 4, 0), (0, 0, 4)), ((0, 0, 0), (0, 4, 0), (0, 0, 4)), ((0, 0, 0), (4, 0, 0), (0, 0, 4)), ((0, 0, 4), (4, 0, 0), (0, 4, 0)),
                ((1.5, 3.75, 1.5), (1, 0, 0), (0, 0, 1))]
    return [NESTED_QUAD]


def inside(points, kind, params):
    """Is each point strictly inside the container?  From the shape's definition: a sphere by its centre and radius; a box through
    the inverse of its instance chain -- Translate takes its offset off, RotateY turns by minus its angle (R/Instance.h:46,121-124)."""
    p = np.asarray(points, dtype=np.float64)
    if kind == "sphere":
        centre, radius = params
        return np.linalg.norm(p - np.asarray(centre), axis=-1) < radius
    lo, hi, degrees, offset = params
    q = p - np.asarray(offset)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    local = np.stack([c * q[:, 0] - s * q[:, 2], q[:, 1], s * q[:, 0] + c * q[:, 2]], axis=-1)
    return np.all((local > np.asarray(lo)) & (local < np.asarray(hi)), axis=-1)


def sample_inside(rng, kind, params, n):
    """n points inside the container, a margin of 2 % away from its surface."""
    if kind == "sphere":
        centre, radius = params
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=-1, keepdims=True)
        return np.asarray(centre) + v * (0.98 * radius * rng.random((n, 1)) ** (1.0 / 3.0))
    lo, hi, degrees, offset = params
    lo, hi = np.asarray(lo), np.asarray(hi)
    local = lo + (0.01 + 0.98 * rng.random((n, 3))) * (hi - lo)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.stack([c * local[:, 0] + s * local[:, 2], local[:, 1], -s * local[:, 0] + c * local[:, 2]], axis=-1) + np.asarray(offset)


# ---- the fixture: tests/golden/reference_hits.npz ----
# Every array is data: ray inputs, the reference's outputs for them, frames, boxes.  To keep the file small the inputs are drawn on
# coarse power-of-two grids (so they are exact in 16-bit integers or fp32 and still exact doubles), and the output rows of a world
# are stored once each, with one index per ray, set and world kind (a miss, a window that changes nothing and the list world beside
# the tree world mostly repeat a row).
SETS = ("free", "inside", "axis", "windows", "times")
FACTORS = np.array([1e-3, 1.0, 1e3])     # the scale of a direction: direction = base * FACTORS[factor]
HIT_FIELDS = (("hit", "u1", ()), ("t", "f8", ()), ("normal", "f8", (3,)), ("uv", "f8", (2,)), ("front_face", "u1", ()), ("material", "u1", ()),
              ("shape", "u1", ()))        # shape: 0 a sphere, 1 a quad or a box face, 2 inside a medium, 255 a miss
STEP_FIELDS = (("status", "u1", ()), ("emitted", "f8", (3,)), ("attenuation", "f8", (3,)), ("origin", "f8", (3,)), ("direction", "f8", (3,)),
               ("time", "f8", ()), ("t", "f8", ()), ("front_face", "u1", ()), ("material", "u1", ()), ("flags", "u1", ()), ("draws", "u2", ()))


def pack(out, key, a):
    """Stores a float64 array under ``key`` in the smallest form that gives every value back bit for bit."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.any(np.signbit(a) & (a == 0)) and np.all(np.isfinite(a)):
        for e in range(-16, 8):
            k = a / 2.0 ** e
            if np.all(k == np.rint(k)) and np.abs(k).max(initial=0) < 32768:
                out[key + ".i16"], out[key + ".q"] = k.astype(np.int16), np.float64(2.0 ** e)
                return
    with np.errstate(over="ignore"):
        narrow = a.astype(np.float32)
    if np.array_equal(narrow.astype(np.float64).view(np.uint64), a.view(np.uint64)):
        out[key + ".f32"] = narrow
    else:
        out[key] = a


def unpack(g, key):
    if key + ".i16" in g:
        return g[key + ".i16"].astype(np.float64) * float(g[key + ".q"])
    if key + ".f32" in g:
        return g[key + ".f32"].astype(np.float64)
    return np.ascontiguousarray(g[key])


def pack_rows(out, key, fields, tables):
    """``tables``: {label: {field: array}} of equally shaped records.  Stores the distinct records once (``key.field``) and an
    index per label (``key@label``)."""
    dtype = np.dtype([(name, kind, tail) for name, kind, tail in fields])
    labels = list(tables)
    rows = []
    for label in labels:
        n = len(tables[label][fields[0][0]])
        r = np.zeros(n, dtype=dtype)
        for name, _, _ in fields:
            r[name] = tables[label][name]
        rows.append(r)
    flat = np.concatenate(rows)
    raw = np.ascontiguousarray(flat).view(np.uint8).reshape(len(flat), dtype.itemsize)
    _, first, inverse = np.unique(raw, axis=0, return_index=True, return_inverse=True)
    order = np.sort(first)                     # the distinct rows in the order they first appear
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    index = rank[inverse.reshape(-1)]
    assert len(order) < 65536
    for name, _, _ in fields:
        out[f"{key}.{name}"] = np.ascontiguousarray(flat[name][order])
    at = 0
    for label, r in zip(labels, rows):
        out[f"{key}@{label}"] = index[at:at + len(r)].astype(np.uint16)
        at += len(r)


def unpack_rows(g, key, fields, label):
    index = g[f"{key}@{label}"].astype(np.int64)
    return {name: np.ascontiguousarray(g[f"{key}.{name}"][index]) for name, _, _ in fields}


def xorwow_advance(state, draws):
    """(n, 6) words {d, v0..v4} after ``draws[k]`` steps of XORWOW each (the step of oracle/rtow_oracle.c xw_next, vectorised)."""
    s = np.array(state, dtype=np.uint32).reshape(-1, 6).copy()
    left = np.array(draws, dtype=np.int64).copy()
    while np.any(left > 0):
        m = left > 0
        d, v = s[m, 0], s[m, 1:].copy()
        t = v[:, 0] ^ (v[:, 0] >> np.uint32(2))
        new = (v[:, 4] ^ (v[:, 4] << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
        s[m, 1:5] = v[:, 1:5]
        s[m, 5] = new
        s[m, 0] = d + np.uint32(362437)
        left[m] -= 1
    return s


class Fixture:
    """tests/golden/reference_hits.npz, unpacked on demand (or a dict of the same arrays, fresh from the generator)."""

    def __init__(self, arrays):
        self.g = arrays

    def rays(self, world, name):
        """(origins, directions, times, tmin, tmax) of a set, float64; ray k of a hit set draws from curand_init(SEED, k, 0)."""
        g, key = self.g, f"{world}/{name}"
        if key + "/again" in g:   # rays of the free and inside sets again
            o, d, _ = self.step_rays(world)
            again = g[key + "/again"].astype(np.int64)
            o, d = np.ascontiguousarray(o[again]), np.ascontiguousarray(d[again])
        else:
            o = unpack(g, key + "/o")
            d = np.ascontiguousarray(unpack(g, key + "/d") * FACTORS[g[key + "/factor"].astype(np.int64)][:, None])
        return o, d, unpack(g, key + "/time"), unpack(g, key + "/tmin"), unpack(g, key + "/tmax")

    def of(self, world, what, kind):
        """frame, boxes, radiance, radiance_exact: the list world's array is stored only where it is not the tree world's."""
        key = f"{world}/{what}{kind}"
        return np.ascontiguousarray(self.g[key if key in self.g else f"{world}/{what}0"])

    def hits(self, world, kind, name):
        return unpack_rows(self.g, f"{world}/hits", HIT_FIELDS, f"{name}{kind}")

    def steps(self, world, kind):
        """The step set: the free rays then the inside rays (default window), ray k with ``streams()[k]``."""
        out = unpack_rows(self.g, f"{world}/steps", STEP_FIELDS, f"{kind}")
        out["rng_state"] = xorwow_advance(self.streams(), out["draws"])
        return out

    def step_rays(self, world):
        (o1, d1, t1, _, _), (o2, d2, t2, _, _) = self.rays(world, "free"), self.rays(world, "inside")
        return np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([t1, t2])

    def streams(self):
        return np.ascontiguousarray(self.g["streams"])
