"""ctypes binding of include/rtow.h.  Fails loudly when the HIP library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTOW_LIB_PATH") or os.path.join(_HERE, "librtow_hip.so")  # override: A/B builds only


class RenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32),
        ("seed", C.c_uint64), ("stripe_rows", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
        ("variant", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32), ("stream", C.c_void_p),
        ("coop_threshold", C.c_int32), ("overdue_rays_per_sample", C.c_int32),
        ("shade_batch", C.c_int32), ("max_blocks_per_cu", C.c_int32), ("pixels_per_wave", C.c_int32), ("reserved0", C.c_int32),
    ]


class RenderStats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64), ("rays", C.c_uint64), ("seconds_seed", C.c_double), ("seconds_render", C.c_double),
        ("pixels", C.c_uint32), ("rows", C.c_uint32), ("kernel_vgprs", C.c_uint32), ("lds_bytes", C.c_uint32),
        ("kernel_kind", C.c_uint32), ("pixels_per_wave", C.c_uint32),
    ]


class AdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_int32), ("check_interval", C.c_int32), ("noise_threshold", C.c_double),
                ("luminance_floor", C.c_double)]


class FeatureParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("seed", C.c_uint64), ("variant", C.c_int32),
                ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_double), ("sigma_albedo", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_depth", C.c_double)]


class QueryParams(C.Structure):
    _fields_ = [("count", C.c_int64), ("tmin", C.c_double), ("tmax", C.c_double), ("time", C.c_double), ("seed", C.c_uint64),
                ("first_sequence", C.c_uint64), ("mode", C.c_int32), ("variant", C.c_int32), ("device", C.c_int32),
                ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class QueryRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origin", "direction", "time", "tmin", "tmax")]


# the outputs of a closest-hit query in the order of rt_query_hits: name -> (numpy dtype, trailing shape)
QUERY_OUTPUTS = {"t": ("float64", ()), "normal": ("float64", (3,)), "uv": ("float64", (2,)), "albedo": ("float64", (3,)),
                 "leaf": ("int32", ()), "front_face": ("uint8", ()), "material": ("uint8", ()), "occluded": ("uint8", ())}


class QueryHits(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in QUERY_OUTPUTS]


class QueryStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32),
                ("scratch_bytes", C.c_uint32)]


class RadianceParams(C.Structure):
    _fields_ = [("count", C.c_int64), ("samples", C.c_int32), ("max_depth", C.c_int32), ("time", C.c_double), ("seed", C.c_uint64),
                ("first_sequence", C.c_uint64), ("variant", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p),
                ("reserved", C.c_int32 * 4)]


class RadianceRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origin", "direction", "time", "rng_state")]


# the outputs of a radiance query in the order of rt_radiance_out: name -> (numpy dtype, trailing shape)
RADIANCE_OUTPUTS = {"radiance": ("float64", (3,)), "path_rays": ("uint32", ()), "rng_state": ("uint32", (6,))}


class RadianceOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RADIANCE_OUTPUTS]


class RadianceStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32), ("scratch_bytes", C.c_uint32)]


# rt_radiance_direct_*: rt_radiance_params field for field and the strategy behind it; the rays and the outputs are the plain call's
class RadianceDirectParams(C.Structure):
    _fields_ = RadianceParams._fields_ + [("strategy", C.c_int32), ("reserved2", C.c_int32 * 3)]


class RadianceDirectStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("shadow_reached", C.c_uint64), ("seconds", C.c_double),
                ("kernel_vgprs", C.c_uint32), ("scratch_bytes", C.c_uint32)]


# rt_render_launch_direct: the strategy of a frame with light samples, and the shadow statistics of the last one finished
class FilmDirectParams(C.Structure):
    _fields_ = [("strategy", C.c_int32), ("reserved", C.c_int32 * 7)]


class FilmDirectStats(C.Structure):
    _fields_ = [("shadow_rays", C.c_uint64), ("shadow_reached", C.c_uint64), ("scratch_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class PathStepParams(C.Structure):
    _fields_ = [("count", C.c_int64), ("time", C.c_double), ("seed", C.c_uint64), ("first_sequence", C.c_uint64), ("variant", C.c_int32),
                ("device", C.c_int32), ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class PathStepRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origin", "direction", "time", "rng_state")]


# the outputs of a path step in the order of rt_path_step_out: name -> (numpy dtype, trailing shape)
STEP_OUTPUTS = {"status": ("uint8", ()), "emitted": ("float64", (3,)), "attenuation": ("float64", (3,)), "origin": ("float64", (3,)),
                "direction": ("float64", (3,)), "time": ("float64", ()), "t": ("float64", ()), "normal": ("float64", (3,)),
                "front_face": ("uint8", ()), "material": ("uint8", ()), "rng_state": ("uint32", (6,))}


class PathStepOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STEP_OUTPUTS]


class PathStepStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("scattered", C.c_uint64), ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32),
                ("scratch_bytes", C.c_uint32)]


class PathAdvanceParams(C.Structure):
    _fields_ = [("count", C.c_int64), ("sources", C.c_int64), ("time", C.c_double), ("seed", C.c_uint64), ("first_sequence", C.c_uint64),
                ("variant", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


class PathAdvanceRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origin", "direction", "time", "rng_state", "throughput", "ray_id", "alive", "count")]


# the per-survivor outputs of a path advance in the order of rt_path_advance_out (without `radiance` in front of them and `count`
# behind): name -> (numpy dtype, trailing shape)
ADVANCE_OUTPUTS = {"origin": ("float64", (3,)), "direction": ("float64", (3,)), "time": ("float64", ()), "rng_state": ("uint32", (6,)),
                   "throughput": ("float64", (3,)), "ray_id": ("int32", ()), "t": ("float64", ()), "normal": ("float64", (3,)),
                   "front_face": ("uint8", ()), "material": ("uint8", ())}


class PathAdvanceOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("radiance",) + tuple(ADVANCE_OUTPUTS) + ("count",)]


class PathAdvanceStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("scattered", C.c_uint64), ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32),
                ("scratch_bytes", C.c_uint32)]


# rt_path_advance_direct_*: the plain advance's structs, field for field, and what the light samples add behind them
class PathAdvanceDirectParams(C.Structure):
    _fields_ = PathAdvanceParams._fields_ + [("strategy", C.c_int32), ("sample", C.c_int32)]


class PathAdvanceDirectRays(C.Structure):
    _fields_ = PathAdvanceRays._fields_ + [("scatter_pdf", C.c_void_p)]


# the per-survivor outputs of a path advance with light samples: the plain advance's and the density the ray was sent with
ADVANCE_DIRECT_OUTPUTS = dict(ADVANCE_OUTPUTS, scatter_pdf=("float64", ()))


class PathAdvanceDirectOut(C.Structure):
    _fields_ = PathAdvanceOut._fields_ + [("scatter_pdf", C.c_void_p)]


class PathAdvanceDirectStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("scattered", C.c_uint64), ("shadow_rays", C.c_uint64), ("shadow_reached", C.c_uint64),
                ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32), ("scratch_bytes", C.c_uint32), ("shadow_vgprs", C.c_uint32),
                ("shadow_scratch_bytes", C.c_uint32)]


class LightParams(C.Structure):
    _fields_ = [("count", C.c_int64), ("time", C.c_double), ("seed", C.c_uint64), ("first_sequence", C.c_uint64), ("strategy", C.c_int32),
                ("variant", C.c_int32), ("device", C.c_int32), ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class LightPoints(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("point", "normal", "material", "time", "rng_state")]


# the outputs of a light sample in the order of rt_light_samples: name -> (numpy dtype, trailing shape)
LIGHT_SAMPLE_OUTPUTS = {"direction": ("float64", (3,)), "distance": ("float64", ()), "light": ("int32", ()), "pdf": ("float64", ()),
                        "emitted": ("float64", (3,)), "scatter_pdf": ("float64", ()), "contribution": ("float64", (3,)),
                        "rng_state": ("uint32", (6,))}


class LightSamples(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LIGHT_SAMPLE_OUTPUTS]


class LightRays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("origin", "direction", "time")]


LIGHT_PDF_OUTPUTS = {"pdf": ("float64", ()), "light": ("int32", ())}


class LightPdfOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LIGHT_PDF_OUTPUTS]


class LightStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("valid", C.c_uint64), ("seconds", C.c_double), ("kernel_vgprs", C.c_uint32),
                ("scratch_bytes", C.c_uint32)]


class Environment(C.Structure):
    """rt_environment: what a miss sees (include/rtow.h rt_scene_set_environment)."""
    _fields_ = [("texture", C.c_uint32), ("rgb", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("intensity", C.c_double * 3),
                ("rotation", C.c_double * 9), ("reserved", C.c_int32 * 4)]


class EnvironmentParams(C.Structure):
    """rt_environment_params: rt_light_params without time and strategy."""
    _fields_ = [("count", C.c_int64), ("seed", C.c_uint64), ("first_sequence", C.c_uint64), ("variant", C.c_int32), ("device", C.c_int32),
                ("stream", C.c_void_p), ("reserved", C.c_int32 * 4)]


class LightRow(C.Structure):
    """rt_light_row: one row of the light table, in world space (include/rtow.h rt_scene_dump_lights)."""
    _fields_ = [("a", C.c_double * 3), ("b", C.c_double * 3), ("c", C.c_double * 3), ("n", C.c_double * 3), ("s", C.c_double),
                ("kind", C.c_uint32), ("mat", C.c_uint32), ("leaf", C.c_uint32), ("pad0", C.c_uint32), ("pad1", C.c_double)]


class LaunchPlan(C.Structure):
    """rt_launch_plan: what a launch decides (csrc/launch_plan.h); every scalar field but ray_budget is an int32."""
    _fields_ = [(n, C.c_uint32 if n == "ray_budget" else C.c_int32) for n in (
        "kernel_kind", "lds_bytes", "pixels_per_wave", "kernel", "probe_kernel", "waves_per_simd", "lds_nodes", "lds_spheres",
        "reference_tree", "always_walk", "accelerate_lists", "coop_threshold", "max_blocks_per_cu", "probe_max_blocks_per_cu",
        "node_burst", "park_ratio", "leaf_batch", "object_batch", "rounds", "shade_batch", "ray_budget",
        "rank_tiles", "pixel_classes", "probe_spp", "tile_flatness_x8", "heavy_threshold", "super_threshold",
        "near_percent", "near_neighbours", "heavy_waves", "heavy_ppw", "super_ppw", "heavy_priority", "adaptive_ppw",
        "lds_front_bytes")] + [("lds_table_offset", C.c_uint32 * 18), ("lds_table_bytes", C.c_uint32 * 18),
                               ("probe_keeps", C.c_int32), ("probe_ray_cap", C.c_int32)]


# the order of rt_launch_plan.lds_table_offset / lds_table_bytes (include/rtow.h RT_LDS_TABLE_NAMES, csrc/launch_plan.h LdsTable)
LDS_TABLES = ("quad_aa", "boxes", "objects", "xforms", "media", "materials", "perlin", "spheres_tab", "group_boxes", "mspheres",
              "msphere_aux", "sphere_aux", "fast_order", "seg_media", "seg_cand", "park", "scan_pairs", "scan_spans")
LDS_GLOBAL = 0xFFFFFFFF   # lds_table_offset of a table the kernel reads from global memory


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "world_kind", "n_leaves", "n_nodes", "n_spheres", "n_moving_spheres", "n_quads", "n_objects", "n_xforms",
        "n_media", "n_materials", "n_textures", "n_perlin", "n_images", "table_bytes", "image_bytes")] + [
        ("reserved", C.c_uint32 * 3)]


H = C.c_uint32
P = C.c_void_p
D = C.c_double
I = C.c_int
D3 = C.POINTER(C.c_double)
I32P = C.POINTER(C.c_int32)


class ObjMesh(C.Structure):  # rt_obj_mesh
    _fields_ = [("vertices", D3), ("normals", D3), ("texcoords", D3), ("indices", I32P), ("normal_indices", I32P), ("texcoord_indices", I32P),
                ("n_vertices", I), ("n_normals", I), ("n_texcoords", I), ("n_triangles", I)]


# name -> (restype, argtypes); exactly the symbols include/rtow.h declares
SIGNATURES = {
    "rt_last_error": (C.c_char_p, []),
    "rt_version": (C.c_char_p, []),
    "rt_rng_create": (P, [C.c_uint64, C.c_uint64]),
    "rt_rng_create_salted": (P, [C.c_uint64, C.c_uint64, I]),
    "rt_rng_destroy": (None, [P]),
    "rt_rng_uniform": (C.c_float, [P]),
    "rt_rng_next_u32": (C.c_uint32, [P]),
    "rt_rng_state": (None, [P, C.POINTER(C.c_uint32)]),
    "rt_rng_create_from_state": (P, [C.POINTER(C.c_uint32)]),
    "rt_scene_create": (P, []),
    "rt_scene_destroy": (None, [P]),
    "rt_scene_set_options": (I, [P, C.c_uint32]),
    "rt_solid_color": (H, [P, D, D, D]),
    "rt_checker_texture": (H, [P, D, H, H]),
    "rt_image_texture": (H, [P, P, I, I]),
    "rt_noise_texture": (H, [P, D, P]),
    "rt_rtwimage_bytes": (None, [P, C.c_size_t, P]),
    "rt_rtwimage_load": (I, [C.c_char_p, C.POINTER(P), C.POINTER(I), C.POINTER(I)]),
    "rt_jpeg_decode": (I, [P, C.c_size_t, C.POINTER(P), C.POINTER(I), C.POINTER(I)]),
    "rt_image_free": (None, [P]),
    "rt_lambertian": (H, [P, D, D, D]),
    "rt_lambertian_tex": (H, [P, H]),
    "rt_metal": (H, [P, D, D, D, D]),
    "rt_dielectric": (H, [P, D]),
    "rt_diffuse_light": (H, [P, D, D, D]),
    "rt_diffuse_light_tex": (H, [P, H]),
    "rt_isotropic": (H, [P, D, D, D]),
    "rt_isotropic_tex": (H, [P, H]),
    "rt_sphere": (H, [P, D, D, D, D, H]),
    "rt_moving_sphere": (H, [P, D, D, D, D, D, D, D, D, D, H]),
    "rt_quad": (H, [P, D3, D3, D3, H]),
    "rt_triangle": (H, [P, D3, D3, D3, H]),
    "rt_triangle_mesh": (H, [P, D3, I, C.POINTER(C.c_int32), I, H, C.POINTER(H)]),
    "rt_obj_load": (I, [C.c_char_p, C.POINTER(D3), C.POINTER(I), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(I)]),
    "rt_mesh_free": (None, [D3, C.POINTER(C.c_int32)]),
    "rt_triangle_attr": (H, [P, D3, D3, D3, D3, D3, H]),
    "rt_triangle_mesh_attr": (H, [P, D3, I, I32P, I, D3, I, I32P, D3, I, I32P, H, C.POINTER(H)]),
    "rt_obj_load_attr": (I, [C.c_char_p, C.POINTER(ObjMesh)]),
    "rt_obj_mesh_free": (None, [C.POINTER(ObjMesh)]),
    "rt_translate": (H, [P, H, D, D, D]),
    "rt_rotate_y": (H, [P, H, D]),
    "rt_transform": (H, [P, H, C.POINTER(C.c_double)]),
    "rt_rotate_x": (H, [P, H, D]),
    "rt_rotate_z": (H, [P, H, D]),
    "rt_scale": (H, [P, H, D, D, D]),
    "rt_transform_get": (C.c_int, [P, H, C.POINTER(C.c_double)]),
    "rt_moving_transform": (H, [P, H, C.POINTER(C.c_double), C.POINTER(C.c_double), D, D]),
    "rt_moving_translate": (H, [P, H, D3, D3, D, D]),
    "rt_moving_transform_get": (C.c_int, [P, H, C.POINTER(C.c_double)]),
    "rt_make_box": (H, [P, D3, D3, H]),
    "rt_hittable_list": (H, [P, C.POINTER(H), I]),
    "rt_constant_medium": (H, [P, H, D, D, D, D]),
    "rt_constant_medium_tex": (H, [P, H, D, H]),
    "rt_bvh_node": (H, [P, C.POINTER(H), I]),
    "rt_hittable_bounding_box": (I, [P, H, D3]),
    "rt_scene_set_world": (I, [P, H]),
    "rt_scene_set_camera": (I, [P, D3, D3, D3, D, D, D, D, D, D, D3]),
    "rt_scene_build_builtin": (I, [P, I, I, I, I, C.c_uint64, P, I, I]),
    "rt_scene_build_sky_demo": (I, [P, I, I, I, C.c_uint64]),
    "rt_scene_commit": (I, [P]),
    "rt_scene_get_info": (I, [P, C.POINTER(SceneInfo)]),
    "rt_scene_dump_leaves": (I, [P, I, C.POINTER(C.c_int), D3]),
    "rt_scene_dump_nodes": (I, [P, I, D3, C.POINTER(C.c_uint32)]),
    "rt_scene_dump_fast_nodes": (I, [P, I, D3, C.POINTER(C.c_uint32), C.POINTER(C.c_uint16)]),
    "rt_scene_dump_camera": (I, [P, D3]),
    "rt_scene_dump_scan_segments": (I, [P, I, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "rt_scene_dump_scan_windows": (I, [P, I, C.POINTER(C.c_uint32), C.POINTER(C.c_float), I, C.POINTER(C.c_float)]),
    "rt_scene_scan_window_trips": (I, [P, I, C.POINTER(C.c_double), C.POINTER(C.c_double), I, C.POINTER(C.c_uint8)]),
    "rt_scene_dump_primary_lists": (I, [P, I, I, I, I, I, I, C.POINTER(C.c_uint16)]),
    "rt_scene_dump_lights": (I, [P, I, C.POINTER(C.c_int), C.POINTER(C.c_int), P, D3]),
    "rt_stripe_rows": (I, [I, I, I, I, C.POINTER(C.c_int), I]),
    "rt_film_create": (P, [I, I, I, I, I, I]),
    "rt_film_destroy": (None, [P]),
    "rt_film_device_pixels": (P, [P]),
    "rt_film_pixel_bytes": (C.c_size_t, [P]),
    "rt_film_bind_pixels": (I, [P, P]),
    "rt_plan_launch": (I, [P, C.POINTER(RenderParams), I, I, C.POINTER(LaunchPlan)]),
    "rt_film_download_probe_costs": (I, [P, C.POINTER(C.c_uint32), I, I]),
    "rt_scene_upload": (I, [P, I]),
    "rt_render_launch": (I, [P, P, C.POINTER(RenderParams)]),
    "rt_render_finish": (I, [P, P, C.POINTER(RenderStats)]),
    "rt_render_launch_direct": (I, [P, P, C.POINTER(RenderParams), C.POINTER(FilmDirectParams)]),
    "rt_film_last_direct_stats": (I, [P, C.POINTER(FilmDirectStats)]),
    "rt_film_direct_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_film_download": (I, [P, D3, I, I]),
    "rt_film_set_adaptive": (I, [P, C.POINTER(AdaptiveParams)]),
    "rt_film_download_sample_counts": (I, [P, C.POINTER(C.c_uint32), I, I]),
    "rt_adaptive_converged": (I, [C.POINTER(AdaptiveParams), C.c_uint32, D, D, D, D]),
    "rt_adaptive_rule_on_device": (I, [I, I, C.POINTER(AdaptiveParams), C.c_uint32, C.POINTER(C.c_uint32), D3, D3, D3, C.POINTER(C.c_uint8)]),
    "rt_film_render_features": (I, [P, P, C.POINTER(FeatureParams)]),
    "rt_film_download_features": (I, [P, D3, D3, D3, I, I]),
    "rt_film_device_features": (P, [P, I]),
    "rt_film_denoise": (I, [P, C.POINTER(DenoiseParams)]),
    "rt_film_download_denoised": (I, [P, D3, I, I]),
    "rt_denoise_frame": (I, [I, D3, D3, D3, D3, I, I, C.POINTER(DenoiseParams), D3]),
    "rt_scene_intersect_device": (I, [P, C.POINTER(QueryParams), C.POINTER(QueryRays), C.POINTER(QueryHits), C.POINTER(QueryStats)]),
    "rt_scene_intersect": (I, [P, C.POINTER(QueryParams), C.POINTER(QueryRays), C.POINTER(QueryHits), C.POINTER(QueryStats)]),
    "rt_query_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_radiance_device": (I, [P, C.POINTER(RadianceParams), C.POINTER(RadianceRays), C.POINTER(RadianceOut), C.POINTER(RadianceStats)]),
    "rt_scene_radiance": (I, [P, C.POINTER(RadianceParams), C.POINTER(RadianceRays), C.POINTER(RadianceOut), C.POINTER(RadianceStats)]),
    "rt_radiance_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_path_step_device": (I, [P, C.POINTER(PathStepParams), C.POINTER(PathStepRays), C.POINTER(PathStepOut), C.POINTER(PathStepStats)]),
    "rt_scene_path_step": (I, [P, C.POINTER(PathStepParams), C.POINTER(PathStepRays), C.POINTER(PathStepOut), C.POINTER(PathStepStats)]),
    "rt_path_step_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_path_advance_device": (I, [P, C.POINTER(PathAdvanceParams), C.POINTER(PathAdvanceRays), C.POINTER(PathAdvanceOut), C.POINTER(PathAdvanceStats)]),
    "rt_scene_path_advance": (I, [P, C.POINTER(PathAdvanceParams), C.POINTER(PathAdvanceRays), C.POINTER(PathAdvanceOut), C.POINTER(PathAdvanceStats)]),
    "rt_path_advance_workspace_bytes": (C.c_uint64, [C.c_int64]),
    "rt_path_advance_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_sample_lights_device": (I, [P, C.POINTER(LightParams), C.POINTER(LightPoints), C.POINTER(LightSamples), C.POINTER(LightStats)]),
    "rt_scene_sample_lights": (I, [P, C.POINTER(LightParams), C.POINTER(LightPoints), C.POINTER(LightSamples), C.POINTER(LightStats)]),
    "rt_scene_light_pdf_device": (I, [P, C.POINTER(LightParams), C.POINTER(LightRays), C.POINTER(LightPdfOut), C.POINTER(LightStats)]),
    "rt_scene_light_pdf": (I, [P, C.POINTER(LightParams), C.POINTER(LightRays), C.POINTER(LightPdfOut), C.POINTER(LightStats)]),
    "rt_light_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_flags": (C.c_uint32, [P]),
    "rt_scene_set_environment": (I, [P, C.POINTER(Environment)]),
    "rt_scene_get_environment": (I, [P, C.POINTER(Environment), C.POINTER(I)]),
    "rt_scene_set_environment_light": (I, [P, C.c_double]),
    "rt_scene_get_environment_light": (I, [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rt_scene_dump_environment_cdf": (I, [P, C.POINTER(I), I, D3, D3]),
    "rt_pfm_load": (I, [C.c_char_p, C.POINTER(P), C.POINTER(I), C.POINTER(I)]),
    "rt_pfm_free": (None, [P]),
    "rt_scene_sample_environment_device": (I, [P, C.POINTER(EnvironmentParams), C.POINTER(LightPoints), C.POINTER(LightSamples), C.POINTER(LightStats)]),
    "rt_scene_sample_environment": (I, [P, C.POINTER(EnvironmentParams), C.POINTER(LightPoints), C.POINTER(LightSamples), C.POINTER(LightStats)]),
    "rt_scene_environment_pdf_device": (I, [P, C.POINTER(EnvironmentParams), C.POINTER(LightRays), C.POINTER(LightPdfOut), C.POINTER(LightStats)]),
    "rt_scene_environment_pdf": (I, [P, C.POINTER(EnvironmentParams), C.POINTER(LightRays), C.POINTER(LightPdfOut), C.POINTER(LightStats)]),
    "rt_environment_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_path_advance_direct_device": (I, [P, C.POINTER(PathAdvanceDirectParams), C.POINTER(PathAdvanceDirectRays), C.POINTER(PathAdvanceDirectOut), C.POINTER(PathAdvanceDirectStats)]),
    "rt_scene_path_advance_direct": (I, [P, C.POINTER(PathAdvanceDirectParams), C.POINTER(PathAdvanceDirectRays), C.POINTER(PathAdvanceDirectOut), C.POINTER(PathAdvanceDirectStats)]),
    "rt_path_advance_direct_workspace_bytes": (C.c_uint64, [C.c_int64]),
    "rt_path_advance_direct_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_scene_radiance_direct_device": (I, [P, C.POINTER(RadianceDirectParams), C.POINTER(RadianceRays), C.POINTER(RadianceOut), C.POINTER(RadianceDirectStats)]),
    "rt_scene_radiance_direct": (I, [P, C.POINTER(RadianceDirectParams), C.POINTER(RadianceRays), C.POINTER(RadianceOut), C.POINTER(RadianceDirectStats)]),
    "rt_radiance_direct_abi_sizes": (None, [C.POINTER(C.c_uint32)]),
    "rt_deinterleave": (I, [D3, I, I, I, I, C.c_size_t, D3]),
    "rt_render": (I, [P, C.POINTER(RenderParams), D3, C.POINTER(RenderStats)]),
    "rt_write_ppm": (I, [C.c_char_p, D3, I, I]),
    "rt_write_ppm_binary": (I, [C.c_char_p, D3, I, I]),
    "rt_write_pfm": (I, [C.c_char_p, D3, I, I]),
}

_lib = None


def load():
    """Load librtow_hip.so.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the render path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export what rtow.h declares
        fn.restype = res
        fn.argtypes = args
    # the radiance, path-step and path-advance structures as this library was compiled against ours: a mismatch would scribble over the
    # caller's arrays
    for what, sizes_of, structs in (("rt_radiance_*", lib.rt_radiance_abi_sizes, (RadianceParams, RadianceRays, RadianceOut, RadianceStats)),
                                    ("rt_path_step_*", lib.rt_path_step_abi_sizes, (PathStepParams, PathStepRays, PathStepOut, PathStepStats)),
                                    ("rt_path_advance_*", lib.rt_path_advance_abi_sizes, (PathAdvanceParams, PathAdvanceRays, PathAdvanceOut, PathAdvanceStats)),
                                    ("rt_path_advance_direct_*", lib.rt_path_advance_direct_abi_sizes,
                                     (PathAdvanceDirectParams, PathAdvanceDirectRays, PathAdvanceDirectOut, PathAdvanceDirectStats)),
                                    ("rt_radiance_direct_*", lib.rt_radiance_direct_abi_sizes,
                                     (RadianceDirectParams, RadianceRays, RadianceOut, RadianceDirectStats))):
        sizes = (C.c_uint32 * 4)()
        sizes_of(sizes)
        ours = [C.sizeof(x) for x in structs]
        if list(sizes) != ours:
            raise ImportError(f"{LIB_PATH}: {what} structures are {list(sizes)} bytes in the library, {ours} in the binding")
    sizes = (C.c_uint32 * 2)()
    lib.rt_film_direct_abi_sizes(sizes)
    ours = [C.sizeof(FilmDirectParams), C.sizeof(FilmDirectStats)]
    if list(sizes) != ours:
        raise ImportError(f"{LIB_PATH}: rt_film_direct_* structures are {list(sizes)} bytes in the library, {ours} in the binding")
    sizes = (C.c_uint32 * 8)()
    lib.rt_light_abi_sizes(sizes)
    ours = [C.sizeof(x) for x in (LightParams, LightPoints, LightSamples, LightRays, LightPdfOut, LightStats, LightRow)]
    if list(sizes)[:7] != ours:
        raise ImportError(f"{LIB_PATH}: rt_light_* structures are {list(sizes)[:7]} bytes in the library, {ours} in the binding")
    sizes = (C.c_uint32 * 4)()
    lib.rt_environment_abi_sizes(sizes)
    ours = [C.sizeof(Environment), C.sizeof(EnvironmentParams)]
    if list(sizes)[:2] != ours:
        raise ImportError(f"{LIB_PATH}: rt_environment* structures are {list(sizes)[:2]} bytes in the library, {ours} in the binding")
    _lib = lib
    return lib


def env_lds_rows():
    """kEnvLdsRows: the entries of the environment's marginal table the sample kernel stages on chip (tests cover both sides of it)."""
    sizes = (C.c_uint32 * 4)()
    load().rt_environment_abi_sizes(sizes)
    return int(sizes[2])


def light_lds_rows():
    """kLightLdsRows: the rows of the light table the light kernels stage on chip (tests cover both sides of it)."""
    sizes = (C.c_uint32 * 8)()
    load().rt_light_abi_sizes(sizes)
    return int(sizes[7])
