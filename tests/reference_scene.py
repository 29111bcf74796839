"""ctypes view of oracle/_ref/libref_world.so: the reference's own classes compiled for the host (oracle/ref_world.cpp), built
by `make -C oracle ref` only where the reference checkout is present.  RefScene and RefRng have conftest.OracleScene's and
OracleRng's method names and argument meanings, so one scene-building callback (query_helpers.mixed_world, reference_worlds.*)
runs on the library, the oracle and the reference.  ``available()`` is false where the library was not built; the tests that need
it skip there and the others read tests/golden/reference_hits.npz, which tests/golden/make_reference_golden.py writes with it."""
import ctypes as C
import functools
import os

import numpy as np

from conftest import ROOT, _d3

PATH = os.path.join(ROOT, "oracle", "_ref", "libref_world.so")
DBL_MAX = float(np.finfo(np.float64).max)


def available():
    return os.path.exists(PATH)


_P, _I, _D, _U64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64
_SIGS = {   # name: (argument types after the scene, result type)
    "ref_c_solid": ([_D] * 3, _I), "ref_c_checker": ([_D, _I, _I], _I), "ref_c_image": ([_P, _I, _I], _I), "ref_c_noise": ([_D, _P], _I),
    "ref_c_lambertian_tex": ([_I], _I), "ref_c_lambertian": ([_D] * 3, _I), "ref_c_metal": ([_D] * 4, _I), "ref_c_dielectric": ([_D], _I),
    "ref_c_light_tex": ([_I], _I), "ref_c_light": ([_D] * 3, _I), "ref_c_isotropic_tex": ([_I], _I), "ref_c_isotropic": ([_D] * 3, _I),
    "ref_c_sphere": ([_D] * 4 + [_I], _I), "ref_c_moving_sphere": ([_D] * 9 + [_I], _I), "ref_c_quad": ([_P] * 3 + [_I], _I),
    "ref_c_translate": ([_I] + [_D] * 3, _I), "ref_c_rotate_y": ([_I, _D], _I), "ref_c_make_box": ([_P, _P, _I], _I),
    "ref_c_list": ([_P, _I], _I), "ref_c_bvh": ([_P, _I], _I), "ref_c_medium": ([_I] + [_D] * 4, _I), "ref_c_medium_tex": ([_I, _D, _I], _I),
    "ref_c_bounding_box": ([_I, _P], _I), "ref_c_set_world": ([_I], _I), "ref_c_set_camera": ([_P] * 3 + [_D] * 6 + [_P], _I),
    "ref_hit": ([_I] + [_P] * 14, _I), "ref_step": ([_I] + [_P] * 14, _I), "ref_render": ([_I, _I, _I, _U64, _P], _I),
}


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(PATH)
    L.ref_new.restype = _P
    L.ref_free.argtypes = [_P]
    L.ref_rng_new.restype, L.ref_rng_new.argtypes = _P, [_U64, _U64]
    L.ref_rng_free.argtypes = [_P]
    L.ref_rng_uniform.restype, L.ref_rng_uniform.argtypes = C.c_float, [_P]
    L.ref_rng_state.argtypes = [_P, _P]
    for name, (args, res) in _SIGS.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = [_P] + args, res
    return L


class RefRng:
    """curand_init(seed, sequence, 0) of oracle/ref_shim/curand_kernel.h."""

    def __init__(self, seed=1984, sequence=0):
        self.L = lib()
        self._p = self.L.ref_rng_new(seed, sequence)

    def __del__(self):
        if getattr(self, "_p", None):
            self.L.ref_rng_free(self._p)
            self._p = None

    def uniform(self):
        return self.L.ref_rng_uniform(self._p)

    def state(self):
        out = np.zeros(6, dtype=np.uint32)
        self.L.ref_rng_state(self._p, out.ctypes.data)
        return [int(x) for x in out]


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a


class RefScene:
    """The reference's object tree built constructor by constructor.  Method names and arguments as conftest.OracleScene."""

    def __init__(self):
        self.L = lib()
        self._p = self.L.ref_new()

    def __del__(self):
        if getattr(self, "_p", None):
            self.L.ref_free(self._p)
            self._p = None

    def _h(self, handle):
        assert handle > 0, "reference constructor call rejected its arguments"
        return handle

    # textures
    def SolidColor(self, c):
        return self._h(self.L.ref_c_solid(self._p, *map(float, c)))

    def CheckerTexture(self, scale, even, odd):
        return self._h(self.L.ref_c_checker(self._p, scale, even, odd))

    def ImageTexture(self, rgb):
        if rgb is None:
            return self._h(self.L.ref_c_image(self._p, None, 0, 0))
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        return self._h(self.L.ref_c_image(self._p, a.ctypes.data, a.shape[1], a.shape[0]))

    def NoiseTexture(self, scale, rng):
        return self._h(self.L.ref_c_noise(self._p, scale, rng._p))

    # materials
    def Lambertian(self, c):
        if isinstance(c, int):
            return self._h(self.L.ref_c_lambertian_tex(self._p, c))
        return self._h(self.L.ref_c_lambertian(self._p, *map(float, c)))

    def Metal(self, c, fuzz):
        return self._h(self.L.ref_c_metal(self._p, float(c[0]), float(c[1]), float(c[2]), fuzz))

    def Dielectric(self, ior):
        return self._h(self.L.ref_c_dielectric(self._p, ior))

    def DiffuseLight(self, c):
        if isinstance(c, int):
            return self._h(self.L.ref_c_light_tex(self._p, c))
        return self._h(self.L.ref_c_light(self._p, *map(float, c)))

    def Isotropic(self, c):
        if isinstance(c, int):
            return self._h(self.L.ref_c_isotropic_tex(self._p, c))
        return self._h(self.L.ref_c_isotropic(self._p, *map(float, c)))

    # hittables
    def Sphere(self, center, radius, material):
        return self._h(self.L.ref_c_sphere(self._p, float(center[0]), float(center[1]), float(center[2]), radius, material))

    def MovingSphere(self, c0, c1, t0, t1, radius, material):
        return self._h(self.L.ref_c_moving_sphere(self._p, *map(float, c0), *map(float, c1), t0, t1, radius, material))

    def Quad(self, q, u, v, material):
        a, b, c = _d3(q), _d3(u), _d3(v)
        return self._h(self.L.ref_c_quad(self._p, C.addressof(a), C.addressof(b), C.addressof(c), material))

    def Translate(self, obj, offset):
        return self._h(self.L.ref_c_translate(self._p, obj, *map(float, offset)))

    def RotateY(self, obj, degrees):
        return self._h(self.L.ref_c_rotate_y(self._p, obj, degrees))

    def MakeBox(self, a, b, material):
        lo, hi = _d3(a), _d3(b)
        return self._h(self.L.ref_c_make_box(self._p, C.addressof(lo), C.addressof(hi), material))

    def HittableList(self, items):
        arr = (C.c_int * max(1, len(items)))(*items)
        return self._h(self.L.ref_c_list(self._p, C.addressof(arr), len(items)))

    def BvhNode(self, items):
        arr = (C.c_int * max(1, len(items)))(*items)
        root = self._h(self.L.ref_c_bvh(self._p, C.addressof(arr), len(items)))
        items[:] = list(arr)[: len(items)]
        return root

    def ConstantMedium(self, boundary, density, c):
        if isinstance(c, int):
            return self._h(self.L.ref_c_medium_tex(self._p, boundary, density, c))
        return self._h(self.L.ref_c_medium(self._p, boundary, density, *map(float, c)))

    def BoundingBox(self, obj):
        out = (C.c_double * 6)()
        assert self.L.ref_c_bounding_box(self._p, obj, C.addressof(out)) == 0
        return list(out)

    def SetWorld(self, world):
        assert self.L.ref_c_set_world(self._p, world) == 0

    def Camera(self, lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=0.0,
               background=(0.70, 0.80, 1.00)):
        a, b, c, d = _d3(lookfrom), _d3(lookat), _d3(vup), _d3(background)
        assert self.L.ref_c_set_camera(self._p, C.addressof(a), C.addressof(b), C.addressof(c), vfov, aspect, aperture,
                                       focus_dist, time0, time1, C.addressof(d)) == 0

    def Commit(self):
        pass

    # batches
    def hit(self, origins, directions, times, tmin, tmax, streams):
        """world->Hit for every ray: per-ray times, windows and six-word streams.  tmax = +inf is passed as DBL_MAX, which is what
        RayColor passes and what the library's queries make of it (include/rtow.h rt_query_params).  Returns a dict: hit, t, p,
        normal, uv, front_face, material_handle, material (the kind, 255 for a miss), rng_state (the streams afterwards)."""
        n = len(origins)
        o, d = _f64(origins, (n, 3)), _f64(directions, (n, 3))
        tm, lo = _f64(np.broadcast_to(times, (n,)), (n,)), _f64(np.broadcast_to(tmin, (n,)), (n,))
        hi = np.minimum(_f64(np.broadcast_to(tmax, (n,)), (n,)), DBL_MAX)
        out = {"rng_state": np.array(streams, dtype=np.uint32).reshape(n, 6), "hit": np.zeros(n, np.uint8), "t": np.zeros(n),
               "p": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "uv": np.zeros((n, 2)), "front_face": np.zeros(n, np.uint8),
               "material_handle": np.zeros(n, np.int32), "material": np.zeros(n, np.uint8)}
        rc = self.L.ref_hit(self._p, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                            *(out[k].ctypes.data for k in ("rng_state", "hit", "t", "p", "normal", "uv", "front_face", "material_handle", "material")))
        assert rc == 0
        return out

    def step(self, origins, directions, times, streams):
        """One iteration of RayColor's loop for every ray, arranged as Scene.path_step arranges it (oracle/ref_world.cpp ref_step).
        Returns a dict: status, emitted, attenuation, origin, direction, time, t, front_face, material, flags (bit 0: a medium
        drew or answered, bit 1: the material reaches a NoiseTexture), rng_state."""
        n = len(origins)
        o, d, tm = _f64(origins, (n, 3)), _f64(directions, (n, 3)), _f64(np.broadcast_to(times, (n,)), (n,))
        out = {"rng_state": np.array(streams, dtype=np.uint32).reshape(n, 6), "status": np.zeros(n, np.uint8), "emitted": np.zeros((n, 3)),
               "attenuation": np.zeros((n, 3)), "origin": np.zeros((n, 3)), "direction": np.zeros((n, 3)), "time": np.zeros(n),
               "t": np.zeros(n), "front_face": np.zeros(n, np.uint8), "material": np.zeros(n, np.uint8), "flags": np.zeros(n, np.uint8)}
        rc = self.L.ref_step(self._p, n, o.ctypes.data, d.ctypes.data, tm.ctypes.data,
                             *(out[k].ctypes.data for k in ("rng_state", "status", "emitted", "attenuation", "origin", "direction", "time", "t",
                                                            "front_face", "material", "flags")))
        assert rc == 0
        return out

    def render(self, W, H, spp, seed=1984):
        fb = np.zeros((H, W, 3), dtype=np.float64)
        assert self.L.ref_render(self._p, W, H, spp, seed, fb.ctypes.data) == 0
        return fb
