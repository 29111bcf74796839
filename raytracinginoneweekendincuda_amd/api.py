"""Host-side mirror of the reference's construction and render interface, over the C-ABI.

Names follow the reference's classes (R/ = reference RayTracinginOneWeekend/): ``Scene.Sphere(center,
radius, material)`` is ``new Sphere(center, radius, material)`` (R/Sphere.h:12), ``Scene.Lambertian``
is R/Material.h:57/63, ``Scene.BvhNode(list)`` is ``new BvhNode(list, 0, n, ...)`` (R/BvhNode.h:50) and
so on; ``Film.render`` is the RenderInit + Render launch pair (R/kernel.cu:675-691) and ``write_ppm`` the
writer at R/kernel.cu:696-721.  Errors surface as RtowError carrying the library's message.
"""
import collections
import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import (AdaptiveParams, DenoiseParams, FeatureParams, FilmDirectParams, FilmDirectStats, LaunchPlan, LightParams, LightPdfOut, LightPoints, LightRays,  # noqa: F401
                   LightSamples, LightStats, QueryHits, QueryParams, QueryRays, QueryStats,  # noqa: F401
                   PathAdvanceOut, PathAdvanceParams, PathAdvanceRays, PathAdvanceStats,
                   PathAdvanceDirectOut, PathAdvanceDirectParams, PathAdvanceDirectRays, PathAdvanceDirectStats,
                   PathStepOut, PathStepParams, PathStepRays, PathStepStats, RadianceOut, RadianceParams, RadianceRays, RadianceStats,
                   RadianceDirectParams, RadianceDirectStats,
                   RenderParams, RenderStats, SceneInfo)


class RtowError(RuntimeError):
    pass


# rt_render_params.flags (include/rtow.h)
FLAG_KEEP_RNG_STATE = 1     # continue the film's saved per-pixel RNG streams (progressive rendering)
FLAG_FORCE_GENERAL = 2      # tests: general kernel even where a specialised instantiation applies
FLAG_OVERDUE_PRIORITY = 4   # diagnostics
FLAG_ACCUMULATE = 8         # with KEEP_RNG_STATE: add this launch's samples to the film's running sums
FLAG_ROW_MAJOR_TILES = 16   # BVH worlds: keep the pixel queue in row-major tile order (no cost ranking)
FLAG_ALWAYS_WALK = 32       # small BVH worlds: walk the tree instead of scanning all leaves
FLAG_ACCELERATE_LISTS = 512  # list worlds of primitives: render through the library's tree (default: scan the list as the reference does)
FLAG_EXACT_SCAN = 256       # sphere-list worlds: the reference's discriminant for every sphere (default: conservative filter first)
FLAG_REFERENCE_TREE = 128   # primitive BVH worlds: walk the reference's own tree (default: the library's SAH tree)
FLAG_FILTER_FP64 = 2048     # sphere-list worlds: the fp64 filter instead of its packed fp32 form (tests, timing)
FLAG_COOP_SINGLE = 1024     # tests: sphere-list worlds, thin waves scan one ray at a time (the older scheme)
FLAG_NO_SCAN_WINDOWS = 8192  # sphere-list worlds: a pass scans every trip of every run (default: the trips its rays can reach; tests, timing)
FLAG_NO_PRIMARY_LISTS = 4096  # sphere-list worlds: camera rays scan the whole list too (default: their tile's candidate list; tests, timing)
FLAG_NO_PIXEL_CLASSES = 64  # sphere-list worlds: one launch for all pixels (no separate launch for the long-chain pixels)


# rt_scene_set_options (read by the next commit)
SCENE_PLAIN_QUADS = 1           # every quad takes the general test; boxes stay lists of six quads
SCENE_REFERENCE_TREE_ONLY = 2   # no library tree for primitive worlds
SCENE_FLAG_ENVIRONMENT = 1024   # Scene.flags(): the committed scene has an environment (rtow.h RT_SCENE_FLAG_ENVIRONMENT)
SCENE_FLAG_ENVIRONMENT_LIGHT = 2048  # ... and direct="mis" samples it as a light (rtow.h RT_SCENE_FLAG_ENVIRONMENT_LIGHT)


# Film.denoise / denoise_frame defaults (DESIGN.md section 5 has the frames they were chosen on)
DENOISE_DEFAULTS = {"iterations": 5, "sigma_color": 0.6, "sigma_albedo": 0.1, "sigma_normal": 0.3, "sigma_depth": 0.1}


def lib():
    return _lib.load()


def library_path():
    return _lib.LIB_PATH


def _err():
    return lib().rt_last_error().decode()


def _check(status):
    if status != 0:
        raise RtowError(f"status {status}: {_err()}")


def _h(handle):
    if not handle:
        raise RtowError(_err())
    return handle


def _v3(v):
    return (C.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))


class Rng:
    """curand_init(seed, sequence, 0) + curand_uniform (R/kernel.cu:101-107, RND at :157)."""

    def __init__(self, seed=1984, sequence=0, salt_kind=0):
        self._p = lib().rt_rng_create_salted(seed, sequence, salt_kind)

    def __del__(self):
        if getattr(self, "_p", None):
            lib().rt_rng_destroy(self._p)
            self._p = None

    def uniform(self):
        return lib().rt_rng_uniform(self._p)

    def next_u32(self):
        return lib().rt_rng_next_u32(self._p)

    def state(self):
        out = (C.c_uint32 * 6)()
        lib().rt_rng_state(self._p, out)
        return list(out)

    @classmethod
    def from_state(cls, words):
        """The stream that continues where ``words`` stood: six 32-bit words {d, v0..v4} as ``state()`` gives them, and as the
        films and the queries return the device streams (include/rtow.h rt_rng_create_from_state)."""
        words = [int(w) & 0xFFFFFFFF for w in words]
        if len(words) != 6:
            raise ValueError("a stream's state is six 32-bit words")
        self = cls.__new__(cls)
        self._p = lib().rt_rng_create_from_state((C.c_uint32 * 6)(*words))
        if not self._p:
            raise RtowError(_err())
        return self


class Scene:
    def __init__(self):
        self._p = lib().rt_scene_create()
        self._keep = []

    def __del__(self):
        if getattr(self, "_p", None):
            lib().rt_scene_destroy(self._p)
            self._p = None

    def set_options(self, options):
        _check(lib().rt_scene_set_options(self._p, options))

    # ---- textures (R/Texture.h) ----
    def SolidColor(self, c):
        return _h(lib().rt_solid_color(self._p, *map(float, c)))

    def CheckerTexture(self, scale, even, odd):
        return _h(lib().rt_checker_texture(self._p, scale, even, odd))

    def ImageTexture(self, rgb):
        if rgb is None:
            return _h(lib().rt_image_texture(self._p, None, 0, 0))
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        return _h(lib().rt_image_texture(self._p, a.ctypes.data, a.shape[1], a.shape[0]))

    def NoiseTexture(self, scale, rng):
        return _h(lib().rt_noise_texture(self._p, scale, rng._p))

    # ---- materials ----
    def Lambertian(self, c):
        if isinstance(c, int):
            return _h(lib().rt_lambertian_tex(self._p, c))
        return _h(lib().rt_lambertian(self._p, *map(float, c)))

    def Metal(self, c, fuzz):
        return _h(lib().rt_metal(self._p, float(c[0]), float(c[1]), float(c[2]), fuzz))

    def Dielectric(self, ior):
        return _h(lib().rt_dielectric(self._p, ior))

    def DiffuseLight(self, c):
        if isinstance(c, int):
            return _h(lib().rt_diffuse_light_tex(self._p, c))
        return _h(lib().rt_diffuse_light(self._p, *map(float, c)))

    def Isotropic(self, c):
        if isinstance(c, int):
            return _h(lib().rt_isotropic_tex(self._p, c))
        return _h(lib().rt_isotropic(self._p, *map(float, c)))

    # ---- hittables ----
    def Sphere(self, center, radius, material):
        return _h(lib().rt_sphere(self._p, float(center[0]), float(center[1]), float(center[2]), radius, material))

    def MovingSphere(self, c0, c1, t0, t1, radius, material):
        return _h(lib().rt_moving_sphere(self._p, *map(float, c0), *map(float, c1), t0, t1, radius, material))

    def Quad(self, q, u, v, material):
        return _h(lib().rt_quad(self._p, _v3(q), _v3(u), _v3(v), material))

    def Triangle(self, q, u, v, material, normals=None, texcoords=None):
        """Corners q, q + u, q + v; the quad's plane and the interior rule 0 <= alpha, 0 <= beta, alpha + beta <= 1 (rtow.h).
        ``normals`` (3, 3): the corners' shading normals, ``texcoords`` (3, 2): their texture coordinates (rt_triangle_attr)."""
        if normals is None and texcoords is None:
            return _h(lib().rt_triangle(self._p, _v3(q), _v3(u), _v3(v), material))
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
        t = None if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float64)
        if (n is not None and n.shape != (3, 3)) or (t is not None and t.shape != (3, 2)):
            raise RtowError("Triangle: normals must be (3, 3) and texcoords (3, 2)")
        return _h(lib().rt_triangle_attr(self._p, _v3(q), _v3(u), _v3(v), None if n is None else n.ctypes.data_as(_lib.D3),
                                         None if t is None else t.ctypes.data_as(_lib.D3), material))

    def TriangleMesh(self, vertices, faces, material, return_triangles=False, normals=None, normal_faces=None, texcoords=None,
                     texcoord_faces=None):
        """A BvhNode over the triangles of an indexed mesh: vertices (N, 3), faces (M, 3) of indices into them (rt_triangle_mesh).
        With ``return_triangles`` also the M triangle handles in input order, for a list or a BvhNode shared with other objects.
        ``normals`` (K, 3) indexed by ``normal_faces`` (M, 3) and ``texcoords`` (L, 2) indexed by ``texcoord_faces`` (M, 3) give
        the corners shading normals and texture coordinates (rt_triangle_mesh_attr); an index array left None is ``faces``."""
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise RtowError("TriangleMesh: vertices must be (N, 3) and faces (M, 3)")
        tris = (C.c_uint32 * max(1, f.shape[0]))()
        i32p = C.POINTER(C.c_int32)
        if normals is None and texcoords is None:
            if normal_faces is not None or texcoord_faces is not None:
                raise RtowError("TriangleMesh: normal_faces / texcoord_faces without normals / texcoords")
            root = _h(lib().rt_triangle_mesh(self._p, v.ctypes.data_as(_lib.D3), v.shape[0], f.ctypes.data_as(i32p), f.shape[0], material, tris))
            return (root, list(tris)[: f.shape[0]]) if return_triangles else root

        def attribute(values, index, width, name):
            if values is None:
                if index is not None:
                    raise RtowError(f"TriangleMesh: {name}_faces without {name}s")
                return None, 0, None, ()
            a = np.ascontiguousarray(values, dtype=np.float64)
            i = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
            if a.ndim != 2 or a.shape[1] != width or (i is not None and i.shape != f.shape):
                raise RtowError(f"TriangleMesh: {name}s must be (K, {width}) and {name}_faces shaped like faces")
            return a.ctypes.data_as(_lib.D3), a.shape[0], None if i is None else i.ctypes.data_as(i32p), (a, i)

        np_, nn, ni, keep_n = attribute(normals, normal_faces, 3, "normal")
        tp, nt, ti, keep_t = attribute(texcoords, texcoord_faces, 2, "texcoord")
        root = _h(lib().rt_triangle_mesh_attr(self._p, v.ctypes.data_as(_lib.D3), v.shape[0], f.ctypes.data_as(i32p), f.shape[0],
                                              np_, nn, ni, tp, nt, ti, material, tris))
        del keep_n, keep_t
        return (root, list(tris)[: f.shape[0]]) if return_triangles else root

    def Translate(self, obj, offset):
        return _h(lib().rt_translate(self._p, obj, *map(float, offset)))

    def RotateY(self, obj, degrees):
        return _h(lib().rt_rotate_y(self._p, obj, degrees))

    @staticmethod
    def _matrix34(matrix, who):
        m = np.array(matrix, dtype=np.float64)
        if m.shape == (4, 4):
            if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
                raise RtowError(f"{who}: the last row of a 4x4 matrix must be 0 0 0 1")
            m = m[:3]
        if m.shape != (3, 4):
            raise RtowError(f"{who}: matrix must be 3x4 or 4x4")
        return np.ascontiguousarray(m)

    def Transform(self, obj, matrix):
        """A general affine instance x_world = L x_obj + t (rt_transform): ``matrix`` is 3x4 ``[L | t]``, or 4x4 with the last row
        0 0 0 1.  Stands wherever Translate / RotateY may stand; rtow.h states its arithmetic operation by operation."""
        m = self._matrix34(matrix, "Transform")
        return _h(lib().rt_transform(self._p, obj, m.ctypes.data_as(C.POINTER(C.c_double))))

    def MovingTransform(self, obj, matrix0, matrix1, time0=0.0, time1=1.0):
        """A moving instance (rt_moving_transform): ``matrix0`` holds at ``time0``, ``matrix1`` at ``time1`` (each as Transform's
        ``matrix``); per ray the two are interpolated entry by entry at the ray's time, clamped to the interval.  Stands wherever a
        Transform may stand; a child that holds a lamp and a matrix that turns singular in between are refused."""
        m0, m1 = self._matrix34(matrix0, "MovingTransform"), self._matrix34(matrix1, "MovingTransform")
        dp = C.POINTER(C.c_double)
        return _h(lib().rt_moving_transform(self._p, obj, m0.ctypes.data_as(dp), m1.ctypes.data_as(dp), float(time0), float(time1)))

    def MovingTranslate(self, obj, offset0, offset1, time0=0.0, time1=1.0):
        """A moving instance whose matrix is the identity: at ``offset0`` at ``time0``, at ``offset1`` at ``time1``."""
        return _h(lib().rt_moving_translate(self._p, obj, _v3(offset0), _v3(offset1), float(time0), float(time1)))

    def moving_transform_keys(self, handle):
        """``(L0, t0, dL, dt, time0, dtime)`` of a moving instance exactly as stored and uploaded (rt_moving_transform_get)."""
        out = (C.c_double * 26)()
        _check(lib().rt_moving_transform_get(self._p, handle, out))
        a = np.array(out, dtype=np.float64)
        return a[:9].reshape(3, 3).copy(), a[9:12].copy(), a[12:21].reshape(3, 3).copy(), a[21:24].copy(), float(a[24]), float(a[25])

    def RotateX(self, obj, degrees):
        return _h(lib().rt_rotate_x(self._p, obj, degrees))

    def RotateZ(self, obj, degrees):
        return _h(lib().rt_rotate_z(self._p, obj, degrees))

    def Scale(self, obj, s):
        """``s``: one factor for the three axes, or three."""
        sx, sy, sz = (float(s),) * 3 if np.ndim(s) == 0 else map(float, s)
        return _h(lib().rt_scale(self._p, obj, sx, sy, sz))

    def transform_matrices(self, handle):
        """``(L, t, Li)`` of a Transform exactly as stored and uploaded: (3, 3), (3,), (3, 3) float64 (rt_transform_get)."""
        out = (C.c_double * 21)()
        _check(lib().rt_transform_get(self._p, handle, out))
        a = np.array(out, dtype=np.float64)
        return a[:9].reshape(3, 3).copy(), a[9:12].copy(), a[12:].reshape(3, 3).copy()

    def MakeBox(self, a, b, material):
        return _h(lib().rt_make_box(self._p, _v3(a), _v3(b), material))

    def HittableList(self, items):
        arr = (C.c_uint32 * max(1, len(items)))(*items)
        return _h(lib().rt_hittable_list(self._p, arr, len(items)))

    def ConstantMedium(self, boundary, density, c):
        if isinstance(c, int):
            return _h(lib().rt_constant_medium_tex(self._p, boundary, density, c))
        return _h(lib().rt_constant_medium(self._p, boundary, density, *map(float, c)))

    def BvhNode(self, items):
        """Sorts ``items`` in place like the reference sorts list[] (R/BvhNode.h:180-193)."""
        arr = (C.c_uint32 * max(1, len(items)))(*items)
        root = _h(lib().rt_bvh_node(self._p, arr, len(items)))
        items[:] = list(arr)[: len(items)]
        return root

    def BoundingBox(self, obj):
        out = (C.c_double * 6)()
        _check(lib().rt_hittable_bounding_box(self._p, obj, out))
        return list(out)

    # ---- world / camera / commit ----
    def SetWorld(self, world):
        _check(lib().rt_scene_set_world(self._p, world))

    def Camera(self, lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=0.0,
               background=(0.70, 0.80, 1.00)):
        _check(lib().rt_scene_set_camera(self._p, _v3(lookfrom), _v3(lookat), _v3(vup), vfov, aspect, aperture,
                                         focus_dist, time0, time1, _v3(background)))

    def Environment(self, texture=None, image=None, intensity=1.0, rotation=None):
        """What a ray that leaves the world sees, in place of the camera's ``background`` (rt_scene_set_environment; rtow.h states
        the lookup operation by operation): a texture handle of this scene -- solid, checker, noise or 8-bit image, looked up at the
        reference's sphere (u, v) of the direction -- or ``image``, a linear float32 H x W x 3 array, top row first (``load_pfm``).
        ``intensity``: one factor or three, per channel.  ``rotation``: 3x3, world -> environment, orthonormal.  Both None: the scene
        goes back to the background.  Takes effect with the next ``Commit``."""
        if texture is None and image is None:
            _check(lib().rt_scene_set_environment(self._p, None))
            return
        env = _lib.Environment()
        env.texture = 0 if texture is None else int(texture)
        a = None
        if image is not None:
            a = np.ascontiguousarray(image, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise RtowError("Environment: image must be H x W x 3")
            env.rgb, env.width, env.height = a.ctypes.data, a.shape[1], a.shape[0]
        k = (float(intensity),) * 3 if np.ndim(intensity) == 0 else tuple(map(float, intensity))
        r = np.eye(3) if rotation is None else np.array(rotation, dtype=np.float64)
        if len(k) != 3 or r.shape != (3, 3):
            raise RtowError("Environment: intensity is one factor or three, rotation 3 x 3")
        env.intensity = (C.c_double * 3)(*k)
        env.rotation = (C.c_double * 9)(*r.reshape(9))
        _check(lib().rt_scene_set_environment(self._p, C.byref(env)))  # (the image is copied)

    def environment(self):
        """The environment as it was set (rt_scene_get_environment): None, or a dict with "texture" (a handle, or None), "image"
        (float32 H x W x 3, or None), "intensity" (3,), "rotation" (3, 3) and "has_distribution": does the committed scene hold the
        importance sampler's tables (``environment_cdf``)."""
        env, has = _lib.Environment(), C.c_int()
        _check(lib().rt_scene_get_environment(self._p, C.byref(env), C.byref(has)))
        if not env.texture and not env.rgb:
            return None
        image = None
        if env.rgb:
            image = np.ctypeslib.as_array(C.cast(env.rgb, C.POINTER(C.c_float)), shape=(env.height, env.width, 3)).copy()
        return {"texture": env.texture or None, "image": image, "intensity": np.array(env.intensity, dtype=np.float64),
                "rotation": np.array(env.rotation, dtype=np.float64).reshape(3, 3), "has_distribution": bool(has.value)}

    def EnvironmentLight(self, chance=0.5):
        """Make the environment a light of ``direct="mis"`` (rt_scene_set_environment_light; rtow.h states the estimator under
        rt_scene_path_advance_direct): a light sample goes to the environment with this chance and to the light table otherwise;
        without lamps every sample goes to the environment.  0 switches it off.  Independent of ``Environment``, without effect
        while the scene has none.  Takes effect with the next ``Commit``; plain renders are not changed by it."""
        _check(lib().rt_scene_set_environment_light(self._p, float(chance)))

    def environment_light(self):
        """``{"chance": as set, "effective": the share c_e of the committed scene}`` (rt_scene_get_environment_light); effective is
        0 before ``Commit``, without an environment and at chance 0, and 1 in a scene without lamps."""
        chance, effective = C.c_double(), C.c_double()
        _check(lib().rt_scene_get_environment_light(self._p, C.byref(chance), C.byref(effective)))
        return {"chance": chance.value, "effective": effective.value}

    def environment_cdf(self):
        """The importance sampler's tables of the committed scene (rt_scene_dump_environment_cdf): ``(marginal (H,), conditional
        (H, W))`` float64, each row ending at exactly 1.0, or None where the environment has no distribution."""
        w = C.c_int()
        h = lib().rt_scene_dump_environment_cdf(self._p, C.byref(w), 0, None, None)
        if h < 0:
            raise RtowError(_err())
        if h == 0:
            return None
        marginal, conditional = np.zeros(h, dtype=np.float64), np.zeros((h, w.value), dtype=np.float64)
        lib().rt_scene_dump_environment_cdf(self._p, C.byref(w), h * w.value, marginal.ctypes.data_as(_lib.D3), conditional.ctypes.data_as(_lib.D3))
        return marginal, conditional

    def flags(self):
        """The committed scene's flags word as the kernels receive it (rt_scene_flags); ``SCENE_FLAG_ENVIRONMENT`` is one bit of it."""
        return int(lib().rt_scene_flags(self._p))

    def Commit(self):
        _check(lib().rt_scene_commit(self._p))

    def build_builtin(self, scene_id, world_kind, width, height, seed=1984, earth=None):
        if earth is not None:
            earth = np.ascontiguousarray(earth, dtype=np.uint8)
            self._keep.append(earth)
            _check(lib().rt_scene_build_builtin(self._p, scene_id, world_kind, width, height, seed, earth.ctypes.data,
                                                earth.shape[1], earth.shape[0]))
        else:
            _check(lib().rt_scene_build_builtin(self._p, scene_id, world_kind, width, height, seed, None, 0, 0))
        return self

    # ---- introspection ----
    def info(self):
        out = SceneInfo()
        _check(lib().rt_scene_get_info(self._p, C.byref(out)))
        info = {n: getattr(out, n) for n, _ in SceneInfo._fields_ if n != "reserved"}
        info["n_triangles"] = out.reserved[0]  # the rows of n_quads that are triangles
        info["n_lights"] = out.reserved[1]     # the rows of the light table (lights())
        info["n_attributed_triangles"] = out.reserved[2]  # the triangle rows with corner normals or texture coordinates
        return info

    def lights(self):
        """The light table (rt_scene_dump_lights; no device needed): every emissive world primitive in world space, in the
        depth-first order of the world, as a dict of arrays with one entry per light -- "kind" (0 quad, 1 triangle, 2 sphere,
        3 moving sphere), "leaf" (the world leaf, as ``intersect`` reports it), "material" (the material row), "a", "b", "c", "n"
        ((n, 3) each) and "s" as include/rtow.h rt_light_row names them, and "cdf" (n, 2): the cumulative selection tables of
        strategy 0 (uniform) and 1 (area x brightest channel), each ending at exactly 1.0."""
        n = lib().rt_scene_dump_lights(self._p, 0, None, None, None, None)
        if n < 0:
            raise RtowError(_err())
        rows = np.zeros(max(n, 1), dtype=np.dtype([("a", "f8", 3), ("b", "f8", 3), ("c", "f8", 3), ("n", "f8", 3), ("s", "f8"), ("kind", "u4"),
                                                   ("mat", "u4"), ("leaf", "u4"), ("pad0", "u4"), ("pad1", "f8")]))
        assert rows.dtype.itemsize == C.sizeof(_lib.LightRow)
        cdf = np.ones((max(n, 1), 2), dtype=np.float64)
        lib().rt_scene_dump_lights(self._p, n, None, None, rows.ctypes.data, cdf.ctypes.data_as(_lib.D3))
        rows = rows[:n]
        out = {name: np.ascontiguousarray(rows[name]) for name in ("a", "b", "c", "n", "s")}
        out.update(kind=rows["kind"].astype(np.int32), leaf=rows["leaf"].astype(np.int32), material=rows["mat"].astype(np.int32), cdf=cdf[:n])
        return out

    def dump_leaves(self):
        n = lib().rt_scene_dump_leaves(self._p, 0, None, None)
        if n < 0:
            raise RtowError(_err())
        kinds = np.zeros(max(n, 1), dtype=np.int32)
        boxes = np.zeros((max(n, 1), 6), dtype=np.float64)
        lib().rt_scene_dump_leaves(self._p, n, kinds.ctypes.data_as(C.POINTER(C.c_int)), boxes.ctypes.data_as(_lib.D3))
        return kinds[:n], boxes[:n]

    def dump_nodes(self):
        n = lib().rt_scene_dump_nodes(self._p, 0, None, None)
        if n < 0:
            raise RtowError(_err())
        boxes = np.zeros((max(n, 1), 6), dtype=np.float64)
        abe = np.zeros((max(n, 1), 3), dtype=np.uint32)
        lib().rt_scene_dump_nodes(self._p, n, boxes.ctypes.data_as(_lib.D3), abe.ctypes.data_as(C.POINTER(C.c_uint32)))
        return boxes[:n], abe[:n]

    def dump_fast_nodes(self):
        """The library's own tree for a primitive-only BVH world: boxes (n, 6), leaf refs (n, 2), octant links (n, 8, 2)."""
        n = lib().rt_scene_dump_fast_nodes(self._p, 0, None, None, None)
        if n < 0:
            raise RtowError(_err())
        boxes = np.zeros((max(n, 1), 6), dtype=np.float64)
        ab = np.zeros((max(n, 1), 2), dtype=np.uint32)
        links = np.zeros((max(n, 1), 8, 2), dtype=np.uint16)
        lib().rt_scene_dump_fast_nodes(self._p, n, boxes.ctypes.data_as(_lib.D3), ab.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       links.ctypes.data_as(C.POINTER(C.c_uint16)))
        return boxes[:n], ab[:n], links[:n]

    def dump_camera(self):
        out = np.zeros(27, dtype=np.float64)
        _check(lib().rt_scene_dump_camera(self._p, out.ctypes.data_as(_lib.D3)))
        return out

    def scan_segments(self):
        """Tests: the segments of the sphere-list scan in list order (rt_scene_dump_scan_segments; no device needed), as a list of
        (first_row, n_rows, axis, shared): axis 0 / 1 / 2 and the fp32 centre coordinate every decided row of a run segment
        shares, or (first_row, n_rows, None, 0.0) for a general segment."""
        n = lib().rt_scene_dump_scan_segments(self._p, 0, None, None)
        if n < 0:
            raise RtowError(_err())
        rows = np.zeros((max(n, 1), 3), dtype=np.uint32)
        shared = np.zeros(max(n, 1), dtype=np.float32)
        lib().rt_scene_dump_scan_segments(self._p, n, rows.ctypes.data_as(C.POINTER(C.c_uint32)), shared.ctypes.data_as(C.POINTER(C.c_float)))
        return [(int(r[0]), int(r[1]), None if r[2] == 3 else int(r[2]), shared[k]) for k, r in enumerate(rows[:n])]

    def scan_windows(self):
        """Tests: the windows of the sphere-list scan's segments (rt_scene_dump_scan_windows; no device needed): a list with one
        entry per segment of scan_segments() -- None for a segment without a table, else (window axis, slab lo, slab hi) -- and
        the spans of all trips of the table as a float32 array (trips, 2)."""
        n = lib().rt_scene_dump_scan_windows(self._p, 0, None, None, 0, None)
        if n < 0:
            raise RtowError(_err())
        trips = lib().rt_scene_scan_window_trips(self._p, 0, None, None, 0, None)
        if trips < 0:
            raise RtowError(_err())
        axis = np.zeros(max(n, 1), dtype=np.uint32)
        slab = np.zeros((max(n, 1), 2), dtype=np.float32)
        spans = np.zeros((max(trips, 1), 2), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        lib().rt_scene_dump_scan_windows(self._p, n, axis.ctypes.data_as(C.POINTER(C.c_uint32)), slab.ctypes.data_as(fp), trips, spans.ctypes.data_as(fp))
        return [None if axis[k] == 3 else (int(axis[k]), slab[k, 0], slab[k, 1]) for k in range(n)], spans[:trips]

    def scan_window_trips(self, origins, directions):
        """Tests: the window rule for rays, one at a time, as the device evaluates it (rt_scene_scan_window_trips; no device
        needed): a bool array (rays, trips), True where the trip must run for the ray.  Trips outside windowed runs are True."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions must have the same shape")
        trips = lib().rt_scene_scan_window_trips(self._p, 0, None, None, 0, None)
        if trips < 0:
            raise RtowError(_err())
        out = np.zeros((o.shape[0], max(trips, 1)), dtype=np.uint8)
        dp = C.POINTER(C.c_double)
        if lib().rt_scene_scan_window_trips(self._p, o.shape[0], o.ctypes.data_as(dp), d.ctypes.data_as(dp), max(trips, 1), out.ctypes.data_as(C.POINTER(C.c_uint8))) < 0:
            raise RtowError(_err())
        return out[:, :trips].astype(bool)

    def primary_lists(self, width, height, stripe_rows=8, rank=0, world_size=1):
        """Tests: the camera rays' candidate lists of a sphere-list world for a film of this geometry (rt_scene_dump_primary_lists;
        no device needed), one per 8x8 tile of the rank's rows, row-major over its compact rows: a list of sphere-list positions
        (ascending), or None for a tile with too many candidates to list."""
        n = lib().rt_scene_dump_primary_lists(self._p, width, height, stripe_rows, rank, world_size, 0, None)
        if n < 0:
            raise RtowError(_err())
        words = np.zeros((max(n, 1), 16), dtype=np.uint16)
        lib().rt_scene_dump_primary_lists(self._p, width, height, stripe_rows, rank, world_size, n, words.ctypes.data_as(C.POINTER(C.c_uint16)))
        return [None if w[0] == 15 else [int(k) for k in w[1:1 + int(w[0])]] for w in words[:n]]

    def plan_launch(self, params, num_cus=256, adaptive=False):
        """Tests: what a launch of this committed scene with these RenderParams decides on a GPU of ``num_cus`` compute units
        -- kernel, LDS, schedule (rt_plan_launch; no device needed).  Returns a dict of the rt_launch_plan fields; the LDS
        layout as ``lds_tables``: {table name: (byte offset in the dynamic LDS block, or None where the kernel reads the
        table from global memory; the table's unpadded bytes)}, behind ``lds_front_bytes`` of node rows or sphere planes."""
        out = LaunchPlan()
        _check(lib().rt_plan_launch(self._p, C.byref(params), num_cus, 1 if adaptive else 0, C.byref(out)))
        plan = {n: getattr(out, n) for n, _ in LaunchPlan._fields_ if not n.startswith("lds_table_")}
        plan["lds_tables"] = {name: (None if off == _lib.LDS_GLOBAL else off, size)
                              for name, off, size in zip(_lib.LDS_TABLES, out.lds_table_offset, out.lds_table_bytes)}
        return plan

    def upload(self, device=0):
        _check(lib().rt_scene_upload(self._p, device))

    # ---- caller-supplied rays: the engine under the ray queries, the radiance queries and the path steps ----
    def _ray_batch(self, kind, origins, directions, inputs, outputs, want, calls, structs, stats, device, points_only=False, into=None):
        """One batch of rays through a pair of library entry points, ``calls`` = (on host arrays, on device arrays): numpy arrays
        take the first, torch CUDA tensors the second, in place and on the current stream.  ``inputs``: the optional per-ray arrays as
        (name, value, tail shape, dtype names, scalar_ok); None, or a scalar where ``scalar_ok``, leaves the name to the call's
        parameters.  ``outputs``: the library's table {name: (dtype name, tail shape)} (_lib.*_OUTPUTS), of which ``want`` names
        those to return (``into``: {name: the caller's own array for that output}, checked like an input; the others are
        allocated here).  ``points_only``: the batch has no directions (light samples).
        ``structs(count, rays, outs, device, stream)`` builds the call's three ctypes structs from the addresses
        of the arrays given and wanted; ``stats``: the statistics struct's type, or None.  Returns ({name: output[:count]}, stats)."""
        on_gpu = type(origins).__module__.split(".")[0] == "torch"
        if on_gpu:
            import torch

        def ray_array(name, a, tail, dtypes=("float64",)):
            """A caller's array as the library reads it: C-contiguous, (count,) + tail, one of ``dtypes``.  Nothing is converted or copied."""
            what = dtypes[0] + "".join(f" (or {d})" for d in dtypes[1:])
            if on_gpu:
                if not isinstance(a, torch.Tensor) or not a.is_cuda or a.device != origins.device:
                    raise RtowError(f"{name}: a CUDA tensor on the device of the origins is required")
                if a.dtype not in [getattr(torch, d) for d in dtypes] or not a.is_contiguous():
                    raise RtowError(f"{name}: a contiguous {what} tensor is required (got {a.dtype}, contiguous={a.is_contiguous()})")
            elif not isinstance(a, np.ndarray) or a.dtype not in [np.dtype(d) for d in dtypes] or not a.flags.c_contiguous:
                raise RtowError(f"{name}: a C-contiguous {what} numpy array is required")
            if a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tail:
                raise RtowError(f"{name}: shape {('count',) + tail} is required, got {tuple(a.shape)}")
            return a

        if on_gpu and not (isinstance(origins, torch.Tensor) and origins.is_cuda):
            raise RtowError("origins: torch tensors must live on the GPU (numpy arrays take the host call)")
        arrays = {"origins": ray_array("origins", origins, (3,))}
        count = int(origins.shape[0])
        for name, a, tail, dtypes, scalar_ok in ([] if points_only else [("directions", directions, (3,), ("float64",), False)]) + list(inputs):
            if name != "directions" and (a is None or (scalar_ok and (isinstance(a, numbers.Real) or (isinstance(a, np.ndarray) and a.ndim == 0)))):
                continue   # one value for all rays (a Python or numpy scalar), or none: the call's parameters
            arrays[name] = ray_array(name, a, tail, dtypes)
            if int(a.shape[0]) != count:
                raise RtowError(f"{name}: {int(a.shape[0])} entries for {count} rays")
        unknown = [w for w in want if w not in outputs]
        if unknown:
            raise RtowError(f"unknown {kind} output {unknown[0]!r} (one of {', '.join(outputs)})")

        def address(a):
            return a.data_ptr() if on_gpu else a.ctypes.data

        out = {}
        for name in want:
            dtype, tail = outputs[name]
            shape = (max(count, 1),) + tail   # (never an empty allocation: its address may be null)
            if into and into.get(name) is not None:
                out[name] = ray_array(name + " (output)", into[name], tail, (dtype, "int32") if dtype == "uint32" else (dtype,))
                if int(out[name].shape[0]) != count or count == 0:
                    raise RtowError(f"{name} (output): {count} entries are required (and at least one)")
            elif on_gpu:   # (an output that continues an input, rng_state, has the input's dtype)
                out[name] = torch.empty(shape, dtype=arrays[name].dtype if name in arrays else getattr(torch, dtype), device=origins.device)
            else:
                out[name] = np.empty(shape, dtype=dtype)
        stream = None
        if on_gpu:
            device = origins.device.index if origins.device.index is not None else torch.cuda.current_device()
            stream = torch.cuda.current_stream(origins.device).cuda_stream or None
        p, rays, outs = structs(count, {n: address(a) for n, a in arrays.items()}, {n: address(a) for n, a in out.items()}, int(device), stream)
        st = stats() if stats else None
        _check(calls[on_gpu](self._p, C.byref(p), C.byref(rays), C.byref(outs), C.byref(st) if stats else None))
        return {name: a[:count] for name, a in out.items()}, st

    # ---- ray queries (include/rtow.h rt_scene_intersect) ----
    def _query(self, mode, want, origins, directions, times, tmin, tmax, time, seed, first_sequence, variant, device, stats):
        def structs(count, rays, outs, device, stream):
            p = QueryParams(count, 0.0 if "tmin" in rays else float(tmin), 0.0 if "tmax" in rays else float(tmax), float(time), int(seed),
                            int(first_sequence), mode, int(variant), device, stream)
            return p, QueryRays(*(rays.get(n) for n in ("origins", "directions", "times", "tmin", "tmax"))), QueryHits(**outs)

        inputs = [(name, a, (), ("float64",), True) for name, a in (("times", times), ("tmin", tmin), ("tmax", tmax))]
        return self._ray_batch("query", origins, directions, inputs, _lib.QUERY_OUTPUTS, want, (lib().rt_scene_intersect, lib().rt_scene_intersect_device),
                               structs, QueryStats if stats else None, device)

    def intersect(self, origins, directions, times=None, tmin=0.001, tmax=float("inf"), time=0.0, seed=1984, first_sequence=0,
                  variant=0, want=("t", "normal", "uv", "albedo", "leaf", "front_face", "material"), device=0, stats=False):
        """The closest hit of every ray ``origins[k] + t * directions[k]`` (both (count, 3) float64) over (tmin, tmax): the
        reference's ``world->Hit``, its own tree or list in its own order (include/rtow.h rt_scene_intersect has the rules and what
        each output holds).  ``times``, ``tmin`` and ``tmax`` may each be a (count,) array or one value for all rays.  Returns a
        dict of the outputs named in ``want``; an output that is not asked for costs no work.  numpy arrays take the host call
        and come back as numpy arrays; torch CUDA tensors are read in place, on ``torch.cuda.current_stream()``, and come back as
        tensors on the same device.  Other dtypes and non-contiguous inputs raise RtowError: nothing is converted silently.
        Only a ConstantMedium draws random numbers: ray k from ``curand_init(seed, k + first_sequence, 0)``.  ``stats=True``:
        (outputs, QueryStats)."""
        out, st = self._query(0, tuple(want), origins, directions, times, tmin, tmax, time, seed, first_sequence, variant, device, stats)
        return (out, st) if stats else out

    def occluded(self, origins, directions, times=None, tmin=0.001, tmax=float("inf"), time=0.0, seed=1984, first_sequence=0,
                 variant=0, device=0, stats=False):
        """(count,) bool: does ray k hit anything over (tmin, tmax)?  Exactly ``isfinite(intersect(...)["t"])``; a world without
        media stops at the first accepted hit.  Arguments as for ``intersect``."""
        out, st = self._query(1, ("occluded",), origins, directions, times, tmin, tmax, time, seed, first_sequence, variant, device, stats)
        hit = out["occluded"] != 0
        return (hit, st) if stats else hit

    # ---- radiance queries (include/rtow.h rt_scene_radiance) ----
    def radiance(self, origins, directions, times=None, samples=1, max_depth=50, time=0.0, seed=1984, first_sequence=0, rng_state=None,
                 variant=0, want=("radiance",), device=0, stats=False, direct=None, strategy=1):
        """The light that comes back along every ray ``origins[k] + t * directions[k]`` (both (count, 3) float64): ``samples`` paths
        per ray, each the reference's ``RayColor`` with ``max_depth`` bounces, all from the ray's one stream (include/rtow.h
        rt_scene_radiance has the rules).  ``times`` may be a (count,) array or None (``time`` for all rays).  ``rng_state`` is a
        (count, 6) array of 32-bit words, ``Rng.state()`` per ray, or None: ray k then draws from
        ``curand_init(seed, k + first_sequence, 0)``.  Returns a dict of the outputs named in ``want``: "radiance" (count, 3) float64,
        linear (no gamma, no clamp); "path_rays" (count,) uint32, the world searches of the ray; "rng_state" (count, 6) uint32, the
        stream after its last draw.  numpy arrays take the host call and come back as numpy arrays; torch CUDA tensors are read in
        place, on ``torch.cuda.current_stream()``, and come back as tensors on the same device (``rng_state`` then of dtype uint32 or
        int32; the output has the input's dtype, uint32 without one).  Other dtypes, shapes and non-contiguous inputs raise RtowError:
        nothing is converted silently.  ``stats=True``: (outputs, RadianceStats).
        ``direct="mis"``: every sample is the estimator of ``PathBatch(direct="mis", strategy=strategy).run(max_depth)`` instead --
        a light sample, its shadow ray and the MIS weights at every diffuse hit but the last bounce's -- in the same one launch
        (include/rtow.h rt_scene_radiance_direct); the expectation is the same, "path_rays" counts the path's own searches, and
        ``stats=True`` gives RadianceDirectStats, with the shadow rays.  ``direct=None``: the plain call, whatever ``strategy`` says."""
        if direct not in (None, "mis"):
            raise RtowError('direct must be None or "mis"')
        if direct and strategy not in (0, 1):
            raise RtowError("strategy must be 0 (uniform) or 1 (by area and brightness)")

        def structs(count, rays, outs, device, stream):   # (its own refusals after the engine's, as they always came)
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.RADIANCE_OUTPUTS))
            if not isinstance(samples, numbers.Integral) or not isinstance(max_depth, numbers.Integral):
                raise RtowError("samples and max_depth are integers")
            params = (count, int(samples), int(max_depth), float(time), int(seed), int(first_sequence), int(variant), device, stream)
            p = RadianceDirectParams(*params, (C.c_int32 * 4)(), int(strategy)) if direct else RadianceParams(*params)
            return p, RadianceRays(*(rays.get(n) for n in ("origins", "directions", "times", "rng_state"))), RadianceOut(**outs)

        inputs = [("times", times, (), ("float64",), False), ("rng_state", rng_state, (6,), ("uint32", "int32"), False)]
        calls, stats_type = (lib().rt_scene_radiance, lib().rt_scene_radiance_device), RadianceStats
        if direct:
            calls, stats_type = (lib().rt_scene_radiance_direct, lib().rt_scene_radiance_direct_device), RadianceDirectStats
        out, st = self._ray_batch("radiance", origins, directions, inputs, _lib.RADIANCE_OUTPUTS, tuple(want), calls, structs,
                                  stats_type if stats else None, device)
        return (out, st) if stats else out

    # ---- path steps (include/rtow.h rt_scene_path_step) ----
    def path_step(self, origins, directions, times=None, rng_state=None, time=0.0, seed=1984, first_sequence=0, variant=0,
                  want=("status", "emitted", "attenuation", "origin", "direction", "time", "rng_state"), device=0, stats=False):
        """One bounce of the reference's ``RayColor`` for every ray ``origins[k] + t * directions[k]`` (both (count, 3) float64): the
        world search, then what the material at the hit emits and how it scatters -- one iteration of the loop ``radiance`` runs,
        for an integrator that continues the path itself (include/rtow.h rt_scene_path_step has the rules).  ``times`` and
        ``rng_state`` as for ``radiance``.  Returns a dict of the outputs named in ``want``: "status" (count,) uint8, 0 miss, 1 the
        path ends at this hit, 2 scattered; "emitted" and "attenuation" (count, 3) float64; "origin", "direction" (count, 3) and
        "time" (count,), the scattered ray where status is 2 and the input ray elsewhere; "t", "normal", "front_face", "material" as
        ``intersect`` gives them; "rng_state" (count, 6), the stream after the step's last draw.  Folding ``acc += thr * emitted``
        where status is 0 or 1 and ``thr *= attenuation`` where it is 2, over the rays of status 2, is one sample of ``radiance``.
        numpy arrays take the host call; torch CUDA tensors are read in place, on ``torch.cuda.current_stream()``.  Other dtypes,
        shapes and non-contiguous inputs raise RtowError.  ``stats=True``: (outputs, PathStepStats)."""
        def structs(count, rays, outs, device, stream):
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.STEP_OUTPUTS))
            p = PathStepParams(count, float(time), int(seed), int(first_sequence), int(variant), device, stream)
            return p, PathStepRays(*(rays.get(n) for n in ("origins", "directions", "times", "rng_state"))), PathStepOut(**outs)

        inputs = [("times", times, (), ("float64",), False), ("rng_state", rng_state, (6,), ("uint32", "int32"), False)]
        out, st = self._ray_batch("path step", origins, directions, inputs, _lib.STEP_OUTPUTS, tuple(want),
                                  (lib().rt_scene_path_step, lib().rt_scene_path_step_device), structs, PathStepStats if stats else None, device)
        return (out, st) if stats else out

    # ---- path advances (include/rtow.h rt_scene_path_advance) ----
    def path_advance(self, origins, directions, times=None, rng_state=None, throughput=None, ray_id=None, alive=None, radiance=None,
                     time=0.0, seed=1984, first_sequence=0, variant=0,
                     want=("origin", "direction", "time", "rng_state", "throughput", "ray_id"), device=0, stats=False):
        """One bounce for a batch of paths, with what a loop around ``path_step`` does between two steps done on the device: every
        ray with ``alive[k] != 0`` (all, without ``alive``) is stepped as ``path_step`` steps it; a path that ends adds
        ``throughput[k] * emitted`` to ``radiance[ray_id[k]]``, in place (``radiance``: (sources, 3) float64 or None; an id outside
        0 .. sources - 1 adds nothing; the ids of live rays must be distinct); the scattered rays come back packed, in input order.
        ``throughput`` (count, 3) float64 defaults to ones, ``ray_id`` (count,) int32 to k, ``alive`` is (count,) uint8; ``times`` and
        ``rng_state`` as for ``path_step``.  Returns a dict of the outputs named in ``want``, each cut to the number of survivors:
        "origin", "direction", "time", "rng_state" (the scattered ray and its stream), "throughput" (``throughput[k] * attenuation``),
        "ray_id", and "t", "normal", "front_face", "material" of the hit the survivor scattered from.  The call reads the
        survivors' count, so it waits for the device (``PathBatch`` is the form that does not).  numpy arrays take the host call;
        torch CUDA tensors are read in place, on ``torch.cuda.current_stream()``, with a workspace tensor of this call's own.
        Other dtypes, shapes and non-contiguous inputs raise RtowError.  ``stats=True``: (outputs, PathAdvanceStats)."""
        return self._path_advance(None, origins, directions, times, rng_state, throughput, ray_id, alive, radiance, time, seed, first_sequence,
                                  variant, want, device, stats)

    def path_advance_direct(self, origins, directions, times=None, rng_state=None, throughput=None, ray_id=None, alive=None, radiance=None,
                            scatter_pdf=None, strategy=1, sample=True, time=0.0, seed=1984, first_sequence=0, variant=0,
                            want=("origin", "direction", "time", "rng_state", "throughput", "ray_id", "scatter_pdf"), device=0, stats=False):
        """``path_advance`` with next-event estimation and its MIS weights done in the same call (include/rtow.h
        rt_scene_path_advance_direct states every operation): with ``sample=True`` every ray that scatters from a Lambertian or
        isotropic hit draws one ``sample_lights`` sample from its own stream under ``strategy``, casts its shadow ray and adds the
        sample, weighted ``p_light / (p_light + p_scatter)``, to ``radiance``; a ray that ends on a lamp adds its light weighted
        ``q / (q + p_light)``, where q = ``scatter_pdf[k]`` ((count,) float64, None: zeros) is the density the bounce before sent it
        with -- 0 where no light sample was taken, the lamp then counts in full.  The output "scatter_pdf" is that density for the
        survivors.  ``sample=False`` for the last bounce of a path of fixed length: a light sample stands for the lamp the next
        bounce would find.  Everything else as ``path_advance``.  ``stats=True``: (outputs, PathAdvanceDirectStats)."""
        if strategy not in (0, 1):
            raise RtowError("strategy must be 0 (uniform) or 1 (by area and brightness)")
        return self._path_advance((scatter_pdf, int(strategy), 1 if sample else 0), origins, directions, times, rng_state, throughput, ray_id,
                                  alive, radiance, time, seed, first_sequence, variant, want, device, stats)

    def _path_advance(self, direct, origins, directions, times, rng_state, throughput, ray_id, alive, radiance, time, seed, first_sequence,
                      variant, want, device, stats):
        """Both forms of the advance; ``direct``: None, or (scatter_pdf, strategy, sample) of ``path_advance_direct``."""
        on_gpu = type(origins).__module__.split(".")[0] == "torch"
        wanted = tuple(want)
        outputs = _lib.ADVANCE_DIRECT_OUTPUTS if direct else _lib.ADVANCE_OUTPUTS
        bytes_of = lib().rt_path_advance_direct_workspace_bytes if direct else lib().rt_path_advance_workspace_bytes
        kept = {}   # what the call uses beside the per-ray arrays: alive until the count has been read

        def structs(count, rays, outs, device, stream):
            sources = 0
            if radiance is not None:
                if on_gpu:
                    import torch
                    ok = isinstance(radiance, torch.Tensor) and radiance.is_cuda and radiance.device == origins.device and \
                        radiance.dtype == torch.float64 and radiance.is_contiguous()
                else:
                    ok = isinstance(radiance, np.ndarray) and radiance.dtype == np.float64 and radiance.flags.c_contiguous and radiance.flags.writeable
                if not ok or radiance.ndim != 2 or radiance.shape[1] != 3:
                    raise RtowError("radiance: a contiguous (sources, 3) float64 array of the kind of the origins is required")
                sources = int(radiance.shape[0])
            nbytes = int(bytes_of(count))
            if on_gpu:
                import torch
                kept["count"] = torch.zeros(1, dtype=torch.int32, device=origins.device)
                kept["workspace"] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=origins.device)
                address = lambda a: a.data_ptr()   # noqa: E731
            else:
                kept["count"] = np.zeros(1, dtype=np.uint32)
                address = lambda a: a.ctypes.data   # noqa: E731
            params = (count, sources, float(time), int(seed), int(first_sequence), int(variant), device, stream,
                      address(kept["workspace"]) if on_gpu else None, nbytes if on_gpu else 0)
            ray_arrays = tuple(rays.get(n) for n in ("origins", "directions", "times", "rng_state", "throughput", "ray_id", "alive")) + (None,)
            out_arrays = (address(radiance) if sources else None,) + tuple(outs.get(n) for n in _lib.ADVANCE_OUTPUTS) + (address(kept["count"]),)
            if direct:
                return (PathAdvanceDirectParams(*params, (C.c_int32 * 4)(), direct[1], direct[2]),
                        PathAdvanceDirectRays(*ray_arrays, rays.get("scatter_pdf")), PathAdvanceDirectOut(*out_arrays, outs.get("scatter_pdf")))
            return PathAdvanceParams(*params), PathAdvanceRays(*ray_arrays), PathAdvanceOut(*out_arrays)

        inputs = [("times", times, (), ("float64",), False), ("rng_state", rng_state, (6,), ("uint32", "int32"), False),
                  ("throughput", throughput, (3,), ("float64",), False), ("ray_id", ray_id, (), ("int32",), False),
                  ("alive", alive, (), ("uint8",), False)]
        calls, stats_type = (lib().rt_scene_path_advance, lib().rt_scene_path_advance_device), PathAdvanceStats
        if direct:
            inputs.append(("scatter_pdf", direct[0], (), ("float64",), False))
            calls, stats_type = (lib().rt_scene_path_advance_direct, lib().rt_scene_path_advance_direct_device), PathAdvanceDirectStats
        required = tuple(n for n in ("origin", "direction") if n not in wanted)
        out, st = self._ray_batch("path advance", origins, directions, inputs, outputs, wanted + required, calls, structs,
                                  stats_type if stats else None, device)
        survivors = int(kept["count"][0])   # (a tensor: the copy waits for the stream the call was enqueued on)
        out = {name: out[name][:survivors] for name in wanted}
        return (out, st) if stats else out

    # ---- light sampling queries (include/rtow.h rt_scene_sample_lights, rt_scene_light_pdf) ----
    def sample_lights(self, points, normals=None, materials=None, times=None, rng_state=None, strategy=0, want=None, time=0.0, seed=1984,
                      first_sequence=0, variant=0, device=0, stats=False, out=None):
        """One sample of the scene's emitters (``lights()``) for every point ``points[k]`` ((count, 3) float64), for next-event
        estimation beside ``path_step`` and ``occluded``: a light picked by ``strategy`` (0 uniform, 1 by area x brightness), a
        point on it -- uniform over a quad or triangle, uniform over the cone a sphere subtends -- and the solid-angle density of
        doing so (include/rtow.h rt_scene_sample_lights states every operation).  ``normals`` (count, 3) float64 and ``materials``
        (count,) uint8, as ``path_step`` returns them, are needed for "scatter_pdf" and "contribution"; ``times`` (count,) or ``time``
        place moving spheres; ``rng_state`` as for ``path_step`` (None: point k draws from ``curand_init(seed, k + first_sequence,
        0)``).  Returns a dict of the outputs named in ``want`` (default: all that the inputs allow): "direction" (count, 3), unit;
        "distance"; "light" int32, -1 without lights; "pdf", 0 for an invalid sample; "emitted" (count, 3); "scatter_pdf";
        "contribution" (count, 3) = emitted * scatter_pdf / pdf; "rng_state" (count, 6).  Visibility is the caller's:
        ``occluded(*shadow_rays(points, direction, distance))``.  ``out``: {name: an array of the caller's to write that output into}
        -- "rng_state" may be the input array.  numpy arrays take the host call; torch CUDA tensors are read in place, on
        ``torch.cuda.current_stream()``.  ``stats=True``: (outputs, LightStats)."""
        if want is None:
            want = ("direction", "distance", "light", "pdf", "emitted", "rng_state") + \
                (("scatter_pdf", "contribution") if normals is not None and materials is not None else ())

        def structs(count, rays, outs, device, stream):
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.LIGHT_SAMPLE_OUTPUTS))
            p = LightParams(count, float(time), int(seed), int(first_sequence), int(strategy), int(variant), device, stream)
            return p, LightPoints(*(rays.get(n) for n in ("origins", "normals", "materials", "times", "rng_state"))), LightSamples(**outs)

        inputs = [("normals", normals, (3,), ("float64",), False), ("materials", materials, (), ("uint8",), False),
                  ("times", times, (), ("float64",), False), ("rng_state", rng_state, (6,), ("uint32", "int32"), False)]
        res, st = self._ray_batch("light sample", points, None, inputs, _lib.LIGHT_SAMPLE_OUTPUTS, tuple(want),
                                  (lib().rt_scene_sample_lights, lib().rt_scene_sample_lights_device), structs, LightStats if stats else None, device,
                                  points_only=True, into=out)
        return (res, st) if stats else res

    def light_pdf(self, origins, directions, times=None, strategy=0, want=("pdf",), time=0.0, variant=0, device=0, stats=False):
        """The density with which ``sample_lights`` at ``origins[k]`` produces the direction ``directions[k]`` (both (count, 3)
        float64; the direction need not be unit): the sum over all lights the ray meets of that light's density times its chance
        under ``strategy`` -- the other half of multiple importance sampling, for a scattered ray that finds a lamp.  "light": the
        nearest light met, -1 for none (then "pdf" is 0).  Nothing is drawn.  Arrays as for ``sample_lights``."""
        def structs(count, rays, outs, device, stream):
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.LIGHT_PDF_OUTPUTS))
            p = LightParams(count, float(time), 0, 0, int(strategy), int(variant), device, stream)
            return p, LightRays(*(rays.get(n) for n in ("origins", "directions", "times"))), LightPdfOut(**outs)

        inputs = [("times", times, (), ("float64",), False)]
        res, st = self._ray_batch("light pdf", origins, directions, inputs, _lib.LIGHT_PDF_OUTPUTS, tuple(want),
                                  (lib().rt_scene_light_pdf, lib().rt_scene_light_pdf_device), structs, LightStats if stats else None, device)
        return (res, st) if stats else res

    # ---- environment sampling (include/rtow.h rt_scene_sample_environment, rt_scene_environment_pdf) ----
    def sample_environment(self, points, normals=None, materials=None, rng_state=None, want=None, seed=1984, first_sequence=0, variant=0,
                           device=0, stats=False, out=None):
        """One direction towards the environment for every point ``points[k]``, drawn by the brightness of the map (uniformly over
        the sphere where the environment has no distribution: ``environment()``); include/rtow.h rt_scene_sample_environment states
        every operation.  Arrays and outputs as for ``sample_lights``: "distance" is +inf for a valid sample -- ``shadow_rays`` turns
        it into ``tmax = inf`` --, "light" the texel drawn, row * W + column with rows counted from the top, -1 without a
        distribution; "pdf" and "emitted" are those of the final direction: ``environment_pdf`` of it and what a ``path_step``
        along it returns."""
        if want is None:
            want = ("direction", "distance", "light", "pdf", "emitted", "rng_state") + \
                (("scatter_pdf", "contribution") if normals is not None and materials is not None else ())

        def structs(count, rays, outs, device, stream):
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.LIGHT_SAMPLE_OUTPUTS))
            p = _lib.EnvironmentParams(count, int(seed), int(first_sequence), int(variant), device, stream)
            return p, LightPoints(rays.get("origins"), rays.get("normals"), rays.get("materials"), None, rays.get("rng_state")), LightSamples(**outs)

        inputs = [("normals", normals, (3,), ("float64",), False), ("materials", materials, (), ("uint8",), False),
                  ("rng_state", rng_state, (6,), ("uint32", "int32"), False)]
        res, st = self._ray_batch("environment sample", points, None, inputs, _lib.LIGHT_SAMPLE_OUTPUTS, tuple(want),
                                  (lib().rt_scene_sample_environment, lib().rt_scene_sample_environment_device), structs,
                                  LightStats if stats else None, device, points_only=True, into=out)
        return (res, st) if stats else res

    def environment_pdf(self, origins, directions, want=("pdf",), variant=0, device=0, stats=False):
        """The density with which ``sample_environment`` produces the direction ``directions[k]`` (not necessarily unit; the origin
        does not matter): bit for bit the sampled "pdf" in the strict build.  "light": the texel the direction looks up, -1 without
        a distribution.  Nothing is drawn."""
        def structs(count, rays, outs, device, stream):
            if not outs:
                raise RtowError("want: at least one of " + ", ".join(_lib.LIGHT_PDF_OUTPUTS))
            p = _lib.EnvironmentParams(count, 0, 0, int(variant), device, stream)
            return p, LightRays(rays.get("origins"), rays.get("directions"), None), LightPdfOut(**outs)

        res, st = self._ray_batch("environment pdf", origins, directions, [], _lib.LIGHT_PDF_OUTPUTS, tuple(want),
                                  (lib().rt_scene_environment_pdf, lib().rt_scene_environment_pdf_device), structs,
                                  LightStats if stats else None, device)
        return (res, st) if stats else res

    @staticmethod
    def shadow_rays(points, directions, distances, times=None):
        """The arguments of ``occluded`` for shadow rays towards light samples: ``(points, directions, times, tmin, tmax)`` with
        ``(tmin, tmax) = (0.001, distances * (1 - 2**-20))``.  The rays run along the unit ``directions``, so t is the distance: the
        interval begins where the renderer's own rays begin and ends 2^-20 of the distance short of the lamp -- far above the
        rounding of the sample (a few 2^-52 of it), far below anything a scene resolves.  A stated rule, not a measurement."""
        return points, directions, times, 0.001, distances * (1.0 - 2.0 ** -20)

    # ---- one-call render on one GPU ----
    def render(self, width, height, spp, max_depth=50, seed=1984, variant=0, device=0, flags=0, coop_threshold=0,
               overdue=0, shade_batch=0, max_blocks_per_cu=0, pixels_per_wave=0, adaptive=None, direct=None, strategy=1):
        """``adaptive``: None, or the arguments of ``Film.set_adaptive`` as a tuple / dict -- ``spp`` is then the most
        samples a pixel takes, and the stats carry the per-pixel counts as ``sample_counts`` ((H, W) uint32).
        ``direct="mis"``: every sample is the estimator of ``radiance(direct="mis", strategy=strategy)`` (``Film.launch``); the stats
        then carry ``direct_stats``, the film's FilmDirectStats.  ``direct=None``: the plain render, whatever ``strategy`` says."""
        _direct_or_raise(direct)
        if adaptive is not None or direct is not None:
            film = Film(width, height, device=device)
            if isinstance(adaptive, dict):
                film.set_adaptive(**adaptive)
            elif adaptive is not None:
                film.set_adaptive(*adaptive)
            st = film.render(self, spp, direct=direct, strategy=strategy, max_depth=max_depth, seed=seed, variant=variant, flags=flags,
                             coop_threshold=coop_threshold, overdue=overdue, shade_batch=shade_batch, max_blocks_per_cu=max_blocks_per_cu,
                             pixels_per_wave=pixels_per_wave)
            if adaptive is not None:
                st.sample_counts = film.sample_counts()
            if direct is not None:
                st.direct_stats = film.direct_stats()
            return film.download(), st
        p = RenderParams(width, height, spp, max_depth, seed, 8, 0, 1, variant, device, flags, None, coop_threshold, overdue,
                         shade_batch, max_blocks_per_cu, pixels_per_wave, 0)
        frame = np.zeros((height, width, 3), dtype=np.float64)
        st = RenderStats()
        _check(lib().rt_render(self._p, C.byref(p), frame.ctypes.data_as(_lib.D3), C.byref(st)))
        return frame, st


class PathBatch:
    """A batch of paths that lives on the device (include/rtow.h rt_scene_path_advance_device): two sets of ray tensors, a
    workspace, a one-word count tensor and ``radiance`` ((n, 3) float64, zeros).  ``advance`` enqueues bounces on
    ``torch.cuda.current_stream()`` without the host ever waiting: each call steps the live rays of the current side, folds the
    paths that ended into ``radiance`` and writes the survivors packed, in order, into the other side, which becomes the current
    one.  Takes torch CUDA tensors only: ``origins`` and ``directions`` (n, 3) float64, ``times`` (n,) float64 or None (``time``
    for all), ``rng_state`` (n, 6) uint32 / int32 or None (ray k draws from ``curand_init(seed, k + first_sequence, 0)``).
    The current side's ``origin``, ``direction``, ``time``, ``rng_state``, ``throughput``, ``ray_id`` (and ``t``, ``normal``,
    ``front_face``, ``material`` of the last hit with ``hits=True``) are attributes: tensors of n rows of which the first
    ``live()`` hold the live rays.  A caller may read them and scale ``throughput`` in place (Russian roulette: ``kill`` the
    losers, divide the winners' throughput by their chance).  Work on them on the stream the advances are enqueued on.
    ``direct="mis"``: every advance is a ``Scene.path_advance_direct`` (rt_scene_path_advance_direct_device) under ``strategy`` --
    a light sample, its shadow ray and the MIS weights at every diffuse hit; the sides then hold ``scatter_pdf`` as well, and
    ``run`` takes no light sample at its last bounce.  ``direct=None``: the plain advance."""

    def __init__(self, scene, origins, directions, times=None, rng_state=None, time=0.0, seed=1984, first_sequence=0, variant=0, hits=False,
                 direct=None, strategy=1):
        import torch
        for name, a, tail, dtypes in (("origins", origins, (3,), (torch.float64,)), ("directions", directions, (3,), (torch.float64,)),
                                      ("times", times, (), (torch.float64,)), ("rng_state", rng_state, (6,), (torch.uint32, torch.int32))):
            if a is None and name in ("times", "rng_state"):
                continue
            if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype not in dtypes or not a.is_contiguous():
                raise RtowError(f"{name}: a contiguous CUDA tensor of dtype {' or '.join(str(d) for d in dtypes)} is required")
            if a.device != origins.device or a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tail or a.shape[0] != origins.shape[0]:
                raise RtowError(f"{name}: shape {('count',) + tail} on the device of the origins is required, got {tuple(a.shape)} on {a.device}")
        if variant not in (0, 1):
            raise RtowError("variant must be 0 (strict) or 1 (fast)")
        if direct not in (None, "mis"):
            raise RtowError('direct must be None or "mis"')
        if strategy not in (0, 1):
            raise RtowError("strategy must be 0 (uniform) or 1 (by area and brightness)")
        self.direct = direct
        outputs = _lib.ADVANCE_DIRECT_OUTPUTS if direct else _lib.ADVANCE_OUTPUTS
        self.scene = scene
        self.n = n = int(origins.shape[0])
        self.device = dev = origins.device
        self._index = dev.index if dev.index is not None else torch.cuda.current_device()
        rows = max(n, 1)   # (never an empty allocation: its address may be null)
        names = list(outputs) if hits else ["origin", "direction", "time", "rng_state", "throughput", "ray_id"] + (["scatter_pdf"] if direct else [])
        state_dtype = rng_state.dtype if rng_state is not None else torch.uint32
        kinds = {"float64": torch.float64, "uint32": torch.int32, "int32": torch.int32, "uint8": torch.uint8}
        self._sides = [{name: torch.zeros((rows,) + outputs[name][1], dtype=kinds[outputs[name][0]], device=dev)
                        for name in names} for _ in range(2)]
        for side in self._sides:   # (allocated as int32: the words are the same)
            side["rng_state"] = side["rng_state"].view(state_dtype)
        first = self._sides[0]
        first["origin"][:n] = origins
        first["direction"][:n] = directions
        first["time"][:n] = times if times is not None else float(time)
        first["throughput"].fill_(1.0)
        first["ray_id"][:n] = torch.arange(n, dtype=torch.int32, device=dev)
        if rng_state is not None:
            first["rng_state"].view(torch.int32)[:n] = rng_state.view(torch.int32)
        self._seeded_by_library = rng_state is None   # until the first advance the current side's rng_state holds nothing
        self._current = 0
        self.radiance = torch.zeros((rows, 3), dtype=torch.float64, device=dev)[:n]
        self._count = torch.full((1,), n, dtype=torch.int32, device=dev)
        self._alive = torch.ones(rows, dtype=torch.uint8, device=dev)
        self._killed = False
        nbytes = int((lib().rt_path_advance_direct_workspace_bytes if direct else lib().rt_path_advance_workspace_bytes)(n))
        self._workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        # the structs of a call from side 0 to side 1 and back, built once: the pointers do not change
        self._calls = []
        for src in (0, 1):
            a, b = self._sides[src], self._sides[1 - src]
            params = (n, n, float(time), int(seed), int(first_sequence), int(variant), self._index, None, self._workspace.data_ptr(), nbytes)
            ray_arrays = (a["origin"].data_ptr(), a["direction"].data_ptr(), a["time"].data_ptr(), a["rng_state"].data_ptr(),
                          a["throughput"].data_ptr(), a["ray_id"].data_ptr(), None, self._count.data_ptr())
            out_arrays = (self.radiance.data_ptr() if n else None,) + tuple(b[name].data_ptr() if name in b else None for name in _lib.ADVANCE_OUTPUTS) + \
                (self._count.data_ptr(),)
            if direct:   # (fresh rays: the first side's scatter_pdf is zeros)
                self._calls.append((PathAdvanceDirectParams(*params, (C.c_int32 * 4)(), int(strategy), 1),
                                    PathAdvanceDirectRays(*ray_arrays, a["scatter_pdf"].data_ptr()),
                                    PathAdvanceDirectOut(*out_arrays, b["scatter_pdf"].data_ptr())))
            else:
                self._calls.append((PathAdvanceParams(*params), PathAdvanceRays(*ray_arrays), PathAdvanceOut(*out_arrays)))

    def __getattr__(self, name):   # the current side's tensors
        sides = self.__dict__.get("_sides")
        if sides and name in sides[self._current]:
            return sides[self._current][name]
        raise AttributeError(name)

    def advance(self, bounces=1, capacity=None, stats=False, sample=True):
        """Enqueues ``bounces`` advances on the current stream and returns; nothing waits.  ``capacity``: rows a launch covers, at
        least the live rays' count (``run`` narrows it to a count it has read); None: all n.  ``stats=True`` (measurements): every
        call waits and the list of their PathAdvanceStats (PathAdvanceDirectStats with ``direct``) comes back.  ``sample`` (with
        ``direct`` only): False, these advances draw no light samples -- for the last bounce of a path of fixed length."""
        import torch
        taken = []
        if self.n == 0:
            return taken if stats else None
        capacity = self.n if capacity is None else int(capacity)
        if not 0 < capacity <= self.n:
            raise RtowError(f"capacity must be 1 .. {self.n}")
        stream = torch.cuda.current_stream(self.device).cuda_stream or None
        fn = lib().rt_scene_path_advance_direct_device if self.direct else lib().rt_scene_path_advance_device
        for _ in range(int(bounces)):
            p, rays, out = self._calls[self._current]
            p.count = capacity
            p.stream = stream
            if self.direct:
                p.sample = 1 if sample else 0
            rays.rng_state = None if self._seeded_by_library else self._sides[self._current]["rng_state"].data_ptr()
            rays.alive = self._alive.data_ptr() if self._killed else None
            if stats:
                taken.append(PathAdvanceDirectStats() if self.direct else PathAdvanceStats())
            _check(fn(self.scene._p, C.byref(p), C.byref(rays), C.byref(out), C.byref(taken[-1]) if stats else None))
            if self._killed:
                self._alive.fill_(1)   # (behind the kernels that read the flags, on their stream)
                self._killed = False
            self._seeded_by_library = False
            self._current = 1 - self._current
        return taken if stats else None

    def live(self):
        """The number of live rays: reads the count word, so it waits for the advances enqueued so far."""
        return int(self._count.item()) if self.n else 0

    def kill(self, mask):
        """Drops the rays ``mask`` marks (a bool tensor over the first rows of the current side) at the next advance: they are not
        traced and add nothing to ``radiance``.  The marks are forgotten after that advance."""
        self._alive[:mask.shape[0]].masked_fill_(mask, 0)   # (no wait, unlike an indexed assignment)
        self._killed = True

    def run(self, max_depth, check_every=8):
        """``max_depth`` bounces: the paths still alive after the last are dropped, as ``RayColor`` cuts them, and ``radiance`` is
        ``Scene.radiance(samples=1, max_depth=max_depth)`` of the batch's rays, bit for bit in the strict build.  Every
        ``check_every`` bounces the count is read (a wait) to stop when no ray is left and to narrow later launches to the count;
        0: never, all ``max_depth`` bounces are enqueued at once.  Returns ``radiance``; the caller synchronizes before reading it
        on another stream.  With ``direct`` the radiance is the MIS estimator of the same expectation, and the last bounce takes no
        light sample."""
        done, capacity = 0, self.n
        while done < max_depth and capacity > 0:
            bounces = max_depth - done if check_every <= 0 else min(int(check_every), max_depth - done)
            if self.direct and done + bounces == max_depth:   # the last bounce on its own
                self.advance(bounces - 1, capacity)
                self.advance(1, capacity, sample=False)
            else:
                self.advance(bounces, capacity)
            done += bounces
            if check_every > 0 and done < max_depth:
                capacity = self.live()
        return self.radiance


def scatter_pdf(materials, normals, directions):
    """The solid-angle density with which the renderer's own ``Material::Scatter`` sends a ray from a surface of unit shading
    normal ``normals[k]`` and material kind ``materials[k]`` (as ``intersect`` and ``path_step`` report it) into the unit direction
    ``directions[k]`` -- the closed forms of include/rtow.h rt_scene_sample_lights, for numpy arrays and torch tensors alike:
    Lambertian (0): ``2 cos^3 / pi`` for ``cos = n . d > 0``, else 0 -- the exact density of ``n + uniform point of the unit ball``
    (R/Material.h:67-82; a chord of length ``2 cos`` through a ball of volume ``4 pi / 3``), which is not a cosine lobe;
    isotropic (4): ``1 / (4 pi)``; metal, dielectric, diffuse light and a miss (255): 0, they are treated as specular."""
    pi = 3.1415926535897932385
    c = (normals[..., 0] * directions[..., 0] + normals[..., 1] * directions[..., 1]) + normals[..., 2] * directions[..., 2]
    xp = np
    if type(c).__module__.split(".")[0] == "torch":
        import torch as xp
    zero = xp.zeros_like(c)
    lambertian = xp.where(c > 0, (2.0 * ((c * c) * c)) / pi, zero)
    return xp.where(materials == 0, lambertian, xp.where(materials == 4, zero + 1.0 / (4.0 * pi), zero))


def builtin_scene(scene_id, world_kind, width, height, seed=1984, earth=None):
    """CreateWorld(sceneId) (R/kernel.cu:176-543); world_kind 0 = BvhNode world, 1 = HittableList world."""
    return Scene().build_builtin(scene_id, world_kind, width, height, seed, earth)


def sky_demo_scene(world_kind, width, height, seed=1984):
    """The environment's demonstration scene, ``rtow --scene 15`` (rt_scene_build_sky_demo): the static random spheres on their
    ground under a computed 256 x 128 sky with a small, very bright sun; the camera's background is black.  Committed."""
    s = Scene()
    _check(lib().rt_scene_build_sky_demo(s._p, world_kind, width, height, seed))
    return s


def _direct_or_raise(direct):
    if direct not in (None, "mis"):
        raise ValueError('direct must be None or "mis"')


class Film:
    """frameBuffer + randState of one GPU (R/kernel.cu:606-613), restricted to this rank's row stripes."""

    def __init__(self, width, height, device=0, stripe_rows=8, rank=0, world_size=1):
        self.width, self.height, self.device = width, height, device
        self.stripe_rows, self.rank, self.world_size = stripe_rows, rank, world_size
        self._p = lib().rt_film_create(device, width, height, stripe_rows, rank, world_size)
        if not self._p:
            raise RtowError(_err())

    def __del__(self):
        if getattr(self, "_p", None):
            lib().rt_film_destroy(self._p)   # waits for a launch still in flight
            self._p = None
        self._scene = None

    def params(self, spp, max_depth=50, seed=1984, variant=0, flags=0, stream=None, coop_threshold=0, overdue=0,
               shade_batch=0, max_blocks_per_cu=0, pixels_per_wave=0):
        return RenderParams(self.width, self.height, spp, max_depth, seed, self.stripe_rows, self.rank, self.world_size,
                            variant, self.device, flags, stream, coop_threshold, overdue, shade_batch, max_blocks_per_cu,
                            pixels_per_wave, 0)

    def launch(self, scene, params, direct=None, strategy=1):
        """``direct="mis"``: the frame with light samples (include/rtow.h rt_render_launch_direct) -- every sample of every pixel is
        one sample of ``Scene.radiance(direct="mis", strategy=strategy)`` for the pixel's camera ray, from the pixel's stream; seeds,
        saved streams, running sums, stripes and adaptive sampling are the film's, as for the plain launch, and launches of both
        kinds may follow each other in one frame.  ``direct=None``: the plain launch, whatever ``strategy`` says."""
        _direct_or_raise(direct)
        if direct is None:
            _check(lib().rt_render_launch(scene._p, self._p, C.byref(params)))
        else:
            if not isinstance(strategy, numbers.Integral):
                raise ValueError("strategy must be 0 (uniform) or 1 (by area and brightness)")
            dp = FilmDirectParams(int(strategy))
            _check(lib().rt_render_launch_direct(scene._p, self._p, C.byref(params), C.byref(dp)))
        self._scene = scene   # the kernel reads the scene's tables: keep it alive until finish()

    def finish(self, scene=None):
        st = RenderStats()
        scene = scene if scene is not None else getattr(self, "_scene", None)
        try:
            _check(lib().rt_render_finish(scene._p if scene is not None else None, self._p, C.byref(st)))
        finally:
            self._scene = None
        return st

    def render(self, scene, spp, direct=None, strategy=1, **kw):
        self.launch(scene, self.params(spp, **kw), direct=direct, strategy=strategy)
        return self.finish(scene)

    def direct_stats(self):
        """FilmDirectStats of the last ``direct="mis"`` launch of this film that was finished: shadow rays cast, those that reached
        their lamp, the private memory of the kernel."""
        st = FilmDirectStats()
        _check(lib().rt_film_last_direct_stats(self._p, C.byref(st)))
        return st

    def device_pixels(self):
        return lib().rt_film_device_pixels(self._p), lib().rt_film_pixel_bytes(self._p)

    def bind_pixels(self, device_ptr):
        """Render into caller-owned device memory (a torch tensor's data_ptr()) of pixel_bytes bytes."""
        _check(lib().rt_film_bind_pixels(self._p, device_ptr))

    @property
    def pixel_bytes(self):
        return lib().rt_film_pixel_bytes(self._p)

    def download(self):
        frame = np.zeros((self.height, self.width, 3), dtype=np.float64)
        _check(lib().rt_film_download(self._p, frame.ctypes.data_as(_lib.D3), self.width, self.height))
        return frame

    def set_adaptive(self, min_samples=None, check_interval=None, noise_threshold=None, luminance_floor=0.01):
        """Adaptive sampling for the launches that follow (include/rtow.h rt_film_set_adaptive): a pixel stops at the first
        check point -- min_samples, then every check_interval samples -- where the standard error of its mean is at most
        noise_threshold x max(mean, luminance_floor); the launch's spp is the cap.  ``set_adaptive(None)`` turns it off."""
        if min_samples is None:
            _check(lib().rt_film_set_adaptive(self._p, None))
            return
        p = AdaptiveParams(int(min_samples), int(check_interval), float(noise_threshold), float(luminance_floor))
        _check(lib().rt_film_set_adaptive(self._p, C.byref(p)))

    def sample_counts(self):
        """Samples every pixel has had so far in this frame, (H, W) uint32, row 0 = bottom like ``download``; 0 in rows of
        other ranks.  Without adaptive sampling: the frame's spp everywhere."""
        counts = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(lib().rt_film_download_sample_counts(self._p, counts.ctypes.data_as(C.POINTER(C.c_uint32)), self.width, self.height))
        return counts

    def probe_costs(self):
        """Tests: the rays the rehearsal of the last launch booked per pixel, (H, W) uint32 like ``sample_counts`` -- a pixel it
        stopped at the plan's ``probe_ray_cap`` has at least that many.  Raises where that launch classified no pixels."""
        costs = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(lib().rt_film_download_probe_costs(self._p, costs.ctypes.data_as(C.POINTER(C.c_uint32)), self.width, self.height))
        return costs

    # ---- first-hit feature buffers and the a-trous filter (include/rtow.h) ----
    def render_features(self, scene, samples=0, seed=1984, variant=0, stream=None):
        """Albedo, shading normal and depth of the first hit of every owned pixel into planes the film keeps
        (rt_film_render_features).  ``samples`` 0: one ray through the pixel centre; N >= 1: N primary rays drawn exactly as a
        render of that seed draws them, averaged.  Touches nothing of the frame the film holds."""
        p = FeatureParams(self.width, self.height, int(samples), int(seed), int(variant), stream)
        _check(lib().rt_film_render_features(scene._p, self._p, C.byref(p)))

    def features(self):
        """(albedo (H, W, 3), normal (H, W, 3), depth (H, W)) of the last feature pass, row 0 = bottom like ``download``; 0 in
        rows of other ranks."""
        albedo = np.zeros((self.height, self.width, 3), dtype=np.float64)
        normal = np.zeros((self.height, self.width, 3), dtype=np.float64)
        depth = np.zeros((self.height, self.width), dtype=np.float64)
        _check(lib().rt_film_download_features(self._p, albedo.ctypes.data_as(_lib.D3), normal.ctypes.data_as(_lib.D3),
                                               depth.ctypes.data_as(_lib.D3), self.width, self.height))
        return albedo, normal, depth

    def device_features(self, which):
        """Device pointer of one compact feature plane (0 albedo, 1 normal, 2 depth), or None before the first feature pass."""
        return lib().rt_film_device_features(self._p, which)

    def denoise(self, iterations=DENOISE_DEFAULTS["iterations"], sigma_color=DENOISE_DEFAULTS["sigma_color"],
                sigma_albedo=DENOISE_DEFAULTS["sigma_albedo"], sigma_normal=DENOISE_DEFAULTS["sigma_normal"],
                sigma_depth=DENOISE_DEFAULTS["sigma_depth"]):
        """The edge-avoiding a-trous filter over the film's pixels, guided by its feature planes, into a buffer of its own
        (rt_film_denoise; read it with ``denoised``).  The raw pixels stay as they are.  A sigma of ``inf`` switches its term off."""
        p = DenoiseParams(int(iterations), float(sigma_color), float(sigma_albedo), float(sigma_normal), float(sigma_depth))
        _check(lib().rt_film_denoise(self._p, C.byref(p)))

    def denoised(self):
        frame = np.zeros((self.height, self.width, 3), dtype=np.float64)
        _check(lib().rt_film_download_denoised(self._p, frame.ctypes.data_as(_lib.D3), self.width, self.height))
        return frame


def denoise_frame(color, albedo=None, normal=None, depth=None, iterations=DENOISE_DEFAULTS["iterations"],
                  sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_albedo=DENOISE_DEFAULTS["sigma_albedo"],
                  sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"], device=0):
    """The film's filter on host arrays (rt_denoise_frame): color (H, W, 3); albedo, normal (H, W, 3) and depth (H, W) may each
    be None, that term is then off.  For frames gathered from several ranks and for synthetic inputs."""
    color = np.ascontiguousarray(color, dtype=np.float64)
    assert color.ndim == 3 and color.shape[2] == 3
    h, w = color.shape[:2]

    def guide(a, shape):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == shape
        return a, a.ctypes.data_as(_lib.D3)

    albedo, pa = guide(albedo, (h, w, 3))
    normal, pn = guide(normal, (h, w, 3))
    depth, pz = guide(depth, (h, w))
    out = np.zeros_like(color)
    p = DenoiseParams(int(iterations), float(sigma_color), float(sigma_albedo), float(sigma_normal), float(sigma_depth))
    _check(lib().rt_denoise_frame(device, color.ctypes.data_as(_lib.D3), pa, pn, pz, w, h, C.byref(p), out.ctypes.data_as(_lib.D3)))
    return out


def adaptive_rule_on_device(n, sums_rgbq, sample_rgb, min_samples, check_interval, noise_threshold, luminance_floor=0.01, variant=0, device=0):
    """Tests: the rule as the adaptive render kernels of a build (variant 0 strict, 1 fast) compile it, run on the GPU over arrays
    (rt_adaptive_rule_on_device).  Returns (q + y^2 of the sample, stops) for n (k,), sums_rgbq (k, 4), sample_rgb (k, 3)."""
    n = np.ascontiguousarray(n, dtype=np.uint32)
    sums = np.ascontiguousarray(sums_rgbq, dtype=np.float64)
    sample = np.ascontiguousarray(sample_rgb, dtype=np.float64)
    assert sums.shape == (n.size, 4) and sample.shape == (n.size, 3)
    q_out, stops = np.zeros(n.size, dtype=np.float64), np.zeros(n.size, dtype=np.uint8)
    p = AdaptiveParams(int(min_samples), int(check_interval), float(noise_threshold), float(luminance_floor))
    _check(lib().rt_adaptive_rule_on_device(device, variant, C.byref(p), n.size, n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            sums.ctypes.data_as(_lib.D3), sample.ctypes.data_as(_lib.D3), q_out.ctypes.data_as(_lib.D3),
                                            stops.ctypes.data_as(C.POINTER(C.c_uint8))))
    return q_out, stops.astype(bool)


def adaptive_converged(n, sum_r, sum_g, sum_b, sum_y2, min_samples, check_interval, noise_threshold, luminance_floor=0.01):
    """The stopping rule on the host, from the source the kernel compiles (rt_adaptive_converged): does a pixel with colour
    sums (sum_r, sum_g, sum_b) and sum of squared sample sums sum_y2 stop at n samples?"""
    p = AdaptiveParams(int(min_samples), int(check_interval), float(noise_threshold), float(luminance_floor))
    rc = lib().rt_adaptive_converged(C.byref(p), int(n), float(sum_r), float(sum_g), float(sum_b), float(sum_y2))
    if rc < 0:
        raise RtowError(f"status {-rc}: {_err()}")
    return bool(rc)


def rtwimage_bytes(decoded_rgb):
    """RtwImage::Load's pixel conversion (stb linearisation with gamma 2.2, then FloatToByte): takes decoded 8-bit
    sRGB pixels (H, W, 3) from any JPEG decoder and returns the bytes the reference hands to ImageTexture."""
    a = np.ascontiguousarray(decoded_rgb, dtype=np.uint8)
    out = np.empty_like(a)
    lib().rt_rtwimage_bytes(a.ctypes.data, a.size, out.ctypes.data)
    return out


def _take_image(ptr, w, h):
    try:
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rt_image_free(ptr)


def jpeg_decode(data):
    """The 8-bit sRGB pixels (H, W, 3) of a sequential Huffman JPEG exactly as the reference's stb_image decodes them
    (csrc/jpeg_decode.cpp); raises RtowError for what that restatement does not decode (progressive, CMYK, ...)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    ptr, w, h = C.c_void_p(), C.c_int(), C.c_int()
    _check(lib().rt_jpeg_decode(buf.ctypes.data, buf.size, C.byref(ptr), C.byref(w), C.byref(h)))
    return _take_image(ptr, w, h)


ObjMesh = collections.namedtuple("ObjMesh", "vertices faces normals normal_faces texcoords texcoord_faces")


def load_obj(path, attributes=False):
    """Wavefront OBJ, positions and faces only (rt_obj_load): vertices (N, 3) float64, faces (M, 3) int32, polygons fanned.
    With ``attributes`` (rt_obj_load_attr) an ``ObjMesh`` tuple (vertices, faces, normals (K, 3), normal_faces (M, 3), texcoords
    (L, 2), texcoord_faces (M, 3)) as ``Scene.TriangleMesh`` takes them; a kind that some face corner does not name is None, None."""
    if attributes:
        m = _lib.ObjMesh()
        _check(lib().rt_obj_load_attr(str(path).encode(), C.byref(m)))
        try:
            def take(ptr, rows, width):
                return np.ctypeslib.as_array(ptr, shape=(rows, width)).copy() if ptr else None
            return ObjMesh(take(m.vertices, m.n_vertices, 3), take(m.indices, m.n_triangles, 3),
                           take(m.normals, m.n_normals, 3), take(m.normal_indices, m.n_triangles, 3),
                           take(m.texcoords, m.n_texcoords, 2), take(m.texcoord_indices, m.n_triangles, 3))
        finally:
            lib().rt_obj_mesh_free(C.byref(m))
    v, f = _lib.D3(), C.POINTER(C.c_int32)()
    nv, nf = C.c_int(), C.c_int()
    _check(lib().rt_obj_load(str(path).encode(), C.byref(v), C.byref(nv), C.byref(f), C.byref(nf)))
    try:
        vertices = np.ctypeslib.as_array(v, shape=(nv.value, 3)).copy()
        faces = np.ctypeslib.as_array(f, shape=(nf.value, 3)).copy()
    finally:
        lib().rt_mesh_free(v, f)
    return vertices, faces


def load_image(path):
    """RtwImage::Load (R/RtwImage.h:51-87): the bytes the reference hands to ImageTexture for a JPEG file, bit for bit.
    Returns None if the file cannot be read or decoded, which ImageTexture turns into the reference's cyan fallback."""
    ptr, w, h = C.c_void_p(), C.c_int(), C.c_int()
    if lib().rt_rtwimage_load(str(path).encode(), C.byref(ptr), C.byref(w), C.byref(h)) != 0:
        return None
    return _take_image(ptr, w, h)


def stripe_rows(height, stripe, rank, world_size):
    n = lib().rt_stripe_rows(height, stripe, rank, world_size, None, 0)
    if n < 0:
        raise RtowError("bad stripe arguments")
    rows = (C.c_int * max(n, 1))()
    lib().rt_stripe_rows(height, stripe, rank, world_size, rows, n)
    return list(rows)[:n]


def deinterleave(gathered, width, height, stripe, world_size):
    """gathered: (world_size, rows_max*width*3) float64, as gathered rank-major over RCCL."""
    g = np.ascontiguousarray(gathered, dtype=np.float64)
    frame = np.zeros((height, width, 3), dtype=np.float64)
    _check(lib().rt_deinterleave(g.ctypes.data_as(_lib.D3), width, height, stripe, world_size, g.shape[1],
                                 frame.ctypes.data_as(_lib.D3)))
    return frame


def write_ppm_binary(path, frame):
    f = np.ascontiguousarray(frame, dtype=np.float64)
    _check(lib().rt_write_ppm_binary(str(path).encode(), f.ctypes.data_as(_lib.D3), f.shape[1], f.shape[0]))


def write_pfm(path, frame):
    f = np.ascontiguousarray(frame, dtype=np.float64)
    _check(lib().rt_write_pfm(str(path).encode(), f.ctypes.data_as(_lib.D3), f.shape[1], f.shape[0]))


def load_pfm(path):
    """A colour PFM file as a float32 H x W x 3 array, TOP row first -- what ``Scene.Environment(image=...)`` takes (rt_pfm_load:
    either byte order, the scale's magnitude applied).  ``write_pfm`` writes a frame's rows bottom first, as the format has them:
    ``load_pfm(write_pfm(frame))`` is ``float32(frame[::-1])``."""
    ptr, w, h = C.c_void_p(), C.c_int(), C.c_int()
    _check(lib().rt_pfm_load(str(path).encode(), C.byref(ptr), C.byref(w), C.byref(h)))
    try:
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rt_pfm_free(ptr)


def write_ppm(path, frame):
    f = np.ascontiguousarray(frame, dtype=np.float64)
    _check(lib().rt_write_ppm(str(path).encode(), f.ctypes.data_as(_lib.D3), f.shape[1], f.shape[0]))
