"""Worlds, cameras and a numpy restatement for the camera rays' candidate lists of the sphere-list kernel
(csrc/primary_cull_rule.h), shared by tests/test_primary_lists_host.py and tests/test_primary_lists_gpu.py.  Not a test module."""
import numpy as np

import raytracinginoneweekendincuda_amd as rt

W, H = 64, 48
GROUND = ((0.0, -1000.5, -5.0), 1000.0)
EYE, LOOK = (0.0, 0.3, 0.5), (0.0, 0.0, -5.0)
NO_LIST_AT = (36, 28)  # the pixel through whose centre the row of forty runs: the middle of tile (4, 3) of a 64 x 48 frame


def field(rnd, n):
    return [((float(rnd.uniform(-3, 3)), float(rnd.uniform(-0.4, 1.2)), float(rnd.uniform(-9, -3))), float(rnd.uniform(0.15, 0.45)))
            for _ in range(n)]


def _material(s, k):
    if k % 7 == 0:
        return s.Dielectric(1.5)
    if k % 3 == 0:
        return s.Metal((0.8, 0.6 + 0.03 * (k % 10), 0.5), 0.02 * (k % 8))
    return s.Lambertian((0.1 + 0.08 * (k % 10), 0.5, 0.9 - 0.07 * (k % 11)))


def world(spheres, eye=EYE, look=LOOK, aperture=0.0, focus=10.0, vfov=50.0, aspect=W / H, glass=()):
    """A build function for conftest.build_both: the spheres as a HittableList in this order (those whose position is in `glass`
    are dielectric), and the camera."""
    def build(s, Rng):
        items = [s.Sphere(c, r, s.Dielectric(1.5) if k in glass else _material(s, k)) for k, (c, r) in enumerate(spheres)]
        s.SetWorld(s.HittableList(items))
        s.Camera(eye, look, (0, 1, 0), vfov, aspect, aperture, focus)
        s.Commit()
    return build


def product(build):
    s = rt.Scene()
    build(s, rt.Rng)
    return s


def _axis_through(pixel, eye=EYE, look=LOOK, vfov=50.0, aspect=W / H, focus=10.0):
    """Unit direction of the ray from the eye through the middle of `pixel` of a W x H frame (a pinhole look-at camera)."""
    probe = product(world([GROUND], eye, look, 0.0, focus, vfov, aspect))
    cam = Camera(probe.dump_camera())
    d = cam.llc + (pixel[0] + 0.5) / W * cam.horizontal + (pixel[1] + 0.5) / H * cam.vertical - cam.origin
    return d / np.linalg.norm(d)


def forty_in_a_row():
    """Forty small spheres along the ray through NO_LIST_AT, their images under a pixel wide, on the ground sphere among a few others:
    the tile of that pixel has more candidates than a list holds, its neighbours have lists."""
    axis = _axis_through(NO_LIST_AT)
    row = [(tuple(float(x) for x in np.array(EYE) + (2.0 + k) * axis), 0.03) for k in range(40)]
    rnd = np.random.default_rng(40)
    return [GROUND] + row + field(rnd, 12)


def cases():
    """name -> (spheres in list order, build function).  64 x 48 frames."""
    rnd = np.random.default_rng(20318)
    small = [GROUND] + field(rnd, 47)
    out = {}
    out["field_on_ground"] = (small, world(small))
    sky = [((0.0, -30.0, 40.0), 2.0), ((5.0, 2.0, 30.0), 1.0)]  # both behind the camera and below: no camera ray meets them
    out["sky_only"] = (sky, world(sky))
    inside = small + [(EYE, 0.8)]  # the camera sits at the centre of a glass sphere, the last of the list
    out["camera_inside_glass"] = (inside, world(inside, glass=(len(inside) - 1,)))
    behind = small + [((0.0, 0.6, 6.0), 2.0)]  # wholly behind the camera (which looks down -z from z = 0.5)
    out["sphere_behind_camera"] = (behind, world(behind))
    lens_in = small + [((0.2, 0.3, 0.5), 1.5)]  # contains the whole lens disk of radius 0.5
    out["sphere_contains_lens"] = (lens_in, world(lens_in, aperture=1.0, focus=5.5, glass=(len(lens_in) - 1,)))
    out["lens_zero"] = (small, world(small, aperture=0.0))
    sparse = [GROUND] + field(rnd, 11)  # few enough that even this lens leaves every tile a list
    out["lens_radius_two"] = (sparse, world(sparse, aperture=4.0, focus=5.5))
    row = forty_in_a_row()
    out["forty_in_a_row"] = (row, world(row))
    twins = small[:20] + [((0.3, 0.2, -4.0), 0.6), ((0.3, 0.2, -4.0), 0.6)] + small[20:]  # coincident: the earlier one is seen
    out["coincident_pair"] = (twins, world(twins))
    return out


class Camera:
    """rt_scene_dump_camera as numpy vectors."""

    def __init__(self, dump):
        (self.bg, self.origin, self.llc, self.horizontal, self.vertical, self.u, self.v, self.w) = (np.array(dump[3 * k:3 * k + 3]) for k in range(8))
        self.lens_radius = float(dump[24])

    def rays(self, i, j, xi, eta, px, py, width, height):
        """camera_ray (render.hip) for arrays of pixels, jitters in [0, 1] and lens points of the unit disk: origins, directions."""
        s = ((i + xi) / width)[:, None]
        t = ((j + eta) / height)[:, None]
        o = self.origin + self.lens_radius * (px[:, None] * self.u + py[:, None] * self.v)
        return o, self.llc + s * self.horizontal + t * self.vertical - o


def tile_pixels(tile, width, height, stripe_rows=8, rank=0, world_size=1):
    """Columns and true rows of 8x8 tile `tile` of the rank's compact rows."""
    rows = rt.stripe_rows(height, stripe_rows, rank, world_size)
    tiles_x = (width + 7) // 8
    tx, ty = tile % tiles_x, tile // tiles_x
    return list(range(8 * tx, min(8 * tx + 8, width))), [int(r) for r in rows[8 * ty:8 * ty + 8]]


def tile_rays(cam, cols, rows, width, height, rnd, per_pixel=24):
    """Rays of the tile's border pixels (all of them for a tile this small): jitter at 0 and at 1 and between, lens points on the
    rim, at the centre and inside."""
    border = [(i, j) for i in cols for j in rows if i in (cols[0], cols[-1]) or j in (rows[0], rows[-1])]
    i = np.repeat(np.array([p[0] for p in border], dtype=np.float64), per_pixel)
    j = np.repeat(np.array([p[1] for p in border], dtype=np.float64), per_pixel)
    n = len(i)
    ends = np.array([0.0, 1.0])
    xi = np.where(rnd.random(n) < 0.7, ends[rnd.integers(0, 2, n)], rnd.random(n))
    eta = np.where(rnd.random(n) < 0.7, ends[rnd.integers(0, 2, n)], rnd.random(n))
    phi = rnd.random(n) * 2.0 * np.pi
    rad = np.where(rnd.random(n) < 0.6, 1.0, np.sqrt(rnd.random(n)))
    rad[::7] = 0.0
    return cam.rays(i, j, xi, eta, rad * np.cos(phi), rad * np.sin(phi), width, height)


def reachable(o, d, centres, radii):
    """Per sphere: does some ray's line come within r (1 + 1e-9) of the centre at some t > 0?  (fp64; rays x spheres.)"""
    oc = centres[None, :, :] - o[:, None, :]
    dd = np.sum(d * d, axis=1)[:, None]
    t = np.maximum(np.einsum("nmk,nk->nm", oc, d) / dd, 0.0)
    gap = oc - t[:, :, None] * d[:, None, :]
    dist = np.sqrt(np.sum(gap * gap, axis=2))
    return np.any(dist <= np.abs(radii)[None, :] * (1.0 + 1e-9), axis=0)


def provably_clear(cam, cols, rows, width, height, centre, radius, slack):
    """The rule of primary_cull_rule.h restated without its rounding margins, every bound multiplied by `slack`."""
    s0, s1 = (cols[0] - 1) / width, (cols[-1] + 2) / width
    t0, t1 = (min(rows) - 1) / height, (max(rows) + 2) / height
    sc, tc, hs, ht = 0.5 * (s0 + s1), 0.5 * (t0 + t1), 0.5 * (s1 - s0), 0.5 * (t1 - t0)
    m = cam.llc + sc * cam.horizontal + tc * cam.vertical - cam.origin
    smax = np.linalg.svd(np.stack([cam.u, cam.v], axis=1), compute_uv=False)[0]
    rho_a = abs(cam.lens_radius) * smax
    rho_b = max(np.linalg.norm(hs * cam.horizontal + ht * cam.vertical), np.linalg.norm(hs * cam.horizontal - ht * cam.vertical))
    q, k = slack * (abs(radius) + rho_a), slack * (rho_a + rho_b)
    w = cam.origin - np.array(centre)
    a2, b1, c0 = m @ m - k * k, w @ m - q * k, w @ w - q * q
    return bool(a2 > 0 and c0 > 0 and (b1 >= 0 or c0 * a2 > b1 * b1))
