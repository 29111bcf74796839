"""What the features, ray-query, radiance and triangle tests share: bit views, the centre rays of a scene's camera, the sphere's
closed form and the mixed world (every primitive, texture and material kind, no media)."""
import numpy as np

from conftest import synthetic_earth


def bits(a):
    """float64 as its bit patterns, for bit-for-bit comparison (NaNs and signed zeros included); anything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def centre_rays(scene, width, height):
    """The rays through the pixel centres, which are the samples == 0 rays of the feature pass (and what rtow --pick and
    --radiance-at trace), restated from dump_camera {bg, origin, llc, horizontal, vertical, ...} in centre_ray's order of
    operations, ((llc + u * hor) + v * ver) - origin with u = (i + 0.5) / W, v = (j + 0.5) / H: IEEE double without contraction
    on both sides.  Ray k = j * W + i.  Returns (origins (N, 3), directions (N, 3), time0, background)."""
    cam = scene.dump_camera()
    bg, origin, llc, hor, ver = (cam[3 * k:3 * k + 3] for k in range(5))
    u = ((np.arange(width) + 0.5) / width)[None, :, None]
    v = ((np.arange(height) + 0.5) / height)[:, None, None]
    d = (((llc + u * hor) + v * ver) - origin).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(origin, d.shape)), np.ascontiguousarray(d), float(cam[25]), bg.copy()


def sphere_roots(o, d, centre, radius):
    """R/Sphere.h:28-36: (near root, far root, discriminant relative to b^2); the roots are NaN where the line misses."""
    oc = o - np.asarray(centre, dtype=np.float64)
    a, b, c = dot3(d, d), dot3(oc, d), dot3(oc, oc) - radius * radius
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        root = np.sqrt(disc)
    return (-b - root) / a, (-b + root) / a, disc / (b * b)


def uv_bound(n):
    """What the sphere's U/V may differ by, per hit: they are functions of the unit normal n with |dv/dn| <= 1 / (pi s) and
    |du/dn| <= 1 / (2 pi s), s = sqrt(1 - ny^2) = sqrt(nx^2 + nz^2) (acos and atan2 are ill-conditioned towards the poles).  The
    normals are held to 1e-12; numpy's acos / atan2 and the device's are good to a few ulp of a value in [0, 2 pi]: 1e-14."""
    return (1e-12 / (np.pi * np.sqrt(1.0 - n[:, 1] * n[:, 1])) + 1e-14)[:, None]


def mixed_world(s, Rng, world_kind, aspect):
    """Builds into ``s`` (rt.Scene, conftest.OracleScene or a view of one) with ``Rng`` of its side, as a conftest.build_both
    callback does: ten items of every primitive, texture and material kind, nine small spheres so that the BvhNode world
    (world_kind 0; 1 is the HittableList) is a tree worth the name, and a camera with aperture 0.1 and shutter 0..1, so the lens
    and the time draws count.  Returns ``s``."""
    earth = s.ImageTexture(synthetic_earth())
    checker = s.CheckerTexture(0.6, s.SolidColor((0.2, 0.3, 0.1)), s.SolidColor((0.9, 0.9, 0.9)))
    marble = s.NoiseTexture(4.0, Rng(1984, 0))
    items = [s.Sphere((0, -100.5, -1), 100.0, s.Lambertian(checker)),
             s.Sphere((-1.1, 0.0, -1.2), 0.5, s.Lambertian(earth)),
             s.Sphere((0.0, 0.0, -1.0), 0.5, s.Dielectric(1.5)),
             s.Sphere((1.1, 0.0, -1.2), 0.5, s.Metal((0.8, 0.6, 0.2), 0.3)),
             s.Sphere((0.4, 0.9, -1.6), 0.35, s.Lambertian(marble)),
             s.MovingSphere((-0.6, 0.8, -1.4), (-0.6, 1.1, -1.4), 0.0, 1.0, 0.25, s.Lambertian((0.7, 0.2, 0.2))),
             s.MovingSphere((1.5, 0.7, -0.8), (1.2, 0.7, -0.8), 0.0, 1.0, 0.2, s.Metal((0.9, 0.9, 0.9), 0.0)),
             s.Quad((-2.5, -0.5, -2.5), (5, 0, 0), (0, 2.5, 0), s.Lambertian(earth)),
             s.Quad((-2.4, -0.5, -2.4), (0, 0, 2.5), (0, 1.5, 0.3), s.DiffuseLight((3.0, 2.5, 2.0))),
             s.Quad((2.0, -0.5, 0.2), (0.3, 0, -2.4), (0, 1.2, 0), s.Lambertian(marble))]
    for k in range(9):
        items.append(s.Sphere((-2.0 + 0.5 * k, -0.35, 0.1), 0.15, (s.Lambertian((0.1, 0.2, 0.8)), s.Metal((0.7, 0.7, 0.7), 0.1),
                                                                   s.Isotropic((0.3, 0.9, 0.3)))[k % 3]))
    s.SetWorld(s.BvhNode(items) if world_kind == 0 else s.HittableList(items))
    s.Camera((0.3, 0.7, 2.6), (0, 0.1, -1), (0, 1, 0), 55.0, aspect, 0.1, 3.4, 0.0, 1.0, (0.55, 0.65, 0.9))
    s.Commit()
    return s
