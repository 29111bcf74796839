// launch_plan.h -- every decision of a launch, taken on the host in ONE place: which instantiation of render_kernel runs,
// what it stages in LDS and where, and how the frame is scheduled (tile ranking, heavy / light pixels, serving waves).
// Host-only: no HIP include, no device query, every function a pure function of its arguments -- rt_render_launch
// (device_scene.cpp) and launch_one (render.hip) only carry the result out, and rt_plan_launch (include/rtow.h) shows it to
// tests that have no device.  The frames are bit-identical whatever is decided here; a wrong decision shows up as time only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rtow.h"
#include "flat_scene.h"

namespace rtow {

struct FlatScene;  // scene_host.h

// ---- 1. Kernel kinds: the bits of rt_render_stats.kernel_kind (ABI: tests and callers pin the numbers) ----
enum : int {
    KIND_RICH = 1,            // Perlin-noise or image textures may appear
    KIND_COMPOSITE = 2,       // instances / boxes / lists / media may appear as leaves
    KIND_MEDIA = 4,           // ConstantMedium leaves may appear
    KIND_WORLD = 8,           // x the world: 0 BvhNode world, 1 HittableList world, 2 HittableList of static spheres only
    KIND_NESTED = 32,         // REF_TREE leaves (the interpreter of general nesting)
    KIND_LIBRARY_TREE = 64,   // primitive world walked through the library's own tree
    KIND_GROUPED = 128,       // list scan with the leaves of every ray dealt to several lanes
    KIND_SEGMENTED = 256,     // composite world walked through the library's tree, one walk per run of surfaces between media
    KIND_ADAPTIVE = 512,      // the Adaptive<> form of the instantiation
    KIND_DIRECT = 1024,       // film_direct_kernel: a frame with light samples (rt_render_launch_direct), beside the world's bits
    // The scheduler's predicates look at the bits below KIND_LIBRARY_TREE only (the same kernel is scheduled the same way with
    // or without the bits above).  KIND_NESTED is one of them, so a nested kernel (39, 47) is none of "BVH kernel", "list-scan
    // kernel", "sphere-list kernel": it gets no tile ranking and no pixel classes.  Kept as it has always been: the nested
    // instantiations render scenes no built-in scene and no benchmark contains, nothing has been measured on them, and a
    // frame is the same bit for bit either way.
    KIND_SCHEDULED_BITS = KIND_LIBRARY_TREE - 1,
};
constexpr int kind_scheduled(int kind) { return kind & KIND_SCHEDULED_BITS; }
// a BvhNode world walked as a tree (any leaves, not nested)
constexpr bool is_bvh_kernel(int kind) { return kind_scheduled(kind) < KIND_WORLD; }
// the HittableList of static spheres (C2)
constexpr bool is_sphere_list_kernel(int kind) { return kind_scheduled(kind) >= 2 * KIND_WORLD && kind_scheduled(kind) < KIND_NESTED; }
// a BVH world of primitives only ...
constexpr bool is_prim_bvh_kernel(int kind) { return kind_scheduled(kind) == 0; }
// ... walked through the library's tree (C3)
constexpr bool is_library_tree_prim_kernel(int kind) { return is_prim_bvh_kernel(kind) && (kind & KIND_LIBRARY_TREE) != 0; }
// list scans without media or table textures: leaves can be dealt to lanes (render.hip scan_leaves_grouped)
constexpr bool is_list_scan_kernel(int kind) { return kind_scheduled(kind) == KIND_WORLD || kind_scheduled(kind) == KIND_WORLD + KIND_COMPOSITE; }
// the deep general kernel (one 768-thread workgroup per CU, C5), told from the general kernel of the same kind by the LDS
// only a workgroup that has the CU to itself can ask for
constexpr int kSharedCuLdsMost = 64 * 1024;  // no kernel whose workgroups share a CU stages more than this (lds_layout)
constexpr bool is_deep_kernel(int kind, int lds_bytes)
{
    return kind_scheduled(kind) == KIND_MEDIA + KIND_COMPOSITE + KIND_RICH && lds_bytes > kSharedCuLdsMost;
}

// ---- the instantiations of render_kernel (render.hip: the aliases of Traits<> of the same names) ----
enum KernelId : int {
    K_SPHERE_LIST, K_BVH_PRIMS, K_BVH_PRIMS_FAST,  // group 0 (render.hip RT_GROUP): primitive kernels
    K_LIST_PRIMS, K_LIST_INSTANCES, K_LIST_INSTANCES_5, K_LIST_PRIMS_GROUPED, K_LIST_INSTANCES_GROUPED, K_LIST_GENERAL, K_LIST_NESTED,
    K_BVH_INSTANCES, K_BVH_MEDIA, K_BVH_GENERAL, K_BVH_GENERAL_DEEP, K_BVH_SEGMENTED, K_BVH_NESTED,  // group 1: composite kernels
    K_COUNT,
    K_FIRST_COMPOSITE = K_LIST_PRIMS,
};
// The compile-time properties of an instantiation that a host decision depends on (render.hip Traits<>, which asserts that
// this table and its aliases agree).
struct KernelProps {
    int world;                                       // Traits::WORLD
    bool composite, rich, media, batch, nested;      // ::COMPOSITE, ::RICH, ::MEDIA, ::BATCH, ::NESTED
    int block;                                       // ::BLOCK, threads per workgroup
    bool fast, seg, grouped, park;                   // ::FAST, ::SEG, ::GROUPED, ::PARK
    int min_waves;                                   // ::MIN_WAVES, waves per SIMD the registers leave room for
};
constexpr int kBigBlockThreads = 768;  // workgroups this large run one per CU (render.hip kBigBlock)
constexpr KernelProps kKernelProps[K_COUNT] = {
    /* K_SPHERE_LIST            */ {2, false, false, false, false, false, 256, false, false, false, false, 3},
    /* K_BVH_PRIMS              */ {0, false, false, false, false, false, 256, false, false, false, false, 3},
    /* K_BVH_PRIMS_FAST         */ {0, false, false, false, false, false, 768, true, false, false, false, 3},
    /* K_LIST_PRIMS             */ {1, false, false, false, false, false, 256, false, false, false, false, 4},
    /* K_LIST_INSTANCES         */ {1, true, false, false, false, false, 256, false, false, false, false, 4},
    /* K_LIST_INSTANCES_5       */ {1, true, false, false, false, false, 256, false, false, false, true, 5},
    /* K_LIST_PRIMS_GROUPED     */ {1, false, false, false, false, false, 256, false, false, true, false, 3},
    /* K_LIST_INSTANCES_GROUPED */ {1, true, false, false, false, false, 256, false, false, true, false, 3},
    /* K_LIST_GENERAL           */ {1, true, true, true, false, false, 256, false, false, false, false, 2},
    /* K_LIST_NESTED            */ {1, true, true, true, false, true, 256, false, false, false, false, 2},
    /* K_BVH_INSTANCES          */ {0, true, false, false, false, false, 256, false, false, false, false, 3},
    /* K_BVH_MEDIA              */ {0, true, false, true, false, false, 256, false, false, false, false, 3},
    /* K_BVH_GENERAL            */ {0, true, true, true, false, false, 256, false, false, false, false, 2},
    /* K_BVH_GENERAL_DEEP       */ {0, true, true, true, true, false, 768, false, false, false, false, 3},
    /* K_BVH_SEGMENTED          */ {0, true, true, true, true, false, 768, false, true, false, false, 3},
    /* K_BVH_NESTED             */ {0, true, true, true, false, true, 256, false, false, false, false, 2},
};
constexpr bool same_props(const KernelProps &a, const KernelProps &b)
{
    return a.world == b.world && a.composite == b.composite && a.rich == b.rich && a.media == b.media && a.batch == b.batch &&
           a.nested == b.nested && a.block == b.block && a.fast == b.fast && a.seg == b.seg && a.grouped == b.grouped &&
           a.park == b.park && a.min_waves == b.min_waves;
}
// kind = world * 8 + media * 4 + composite * 2 + rich, + the bits of the special walks (rt_render_stats.kernel_kind)
constexpr int kernel_kind(const KernelProps &k, bool adaptive)
{
    return k.world * KIND_WORLD + (k.media ? KIND_MEDIA : 0) + (k.composite ? KIND_COMPOSITE : 0) + (k.rich ? KIND_RICH : 0) +
           (k.nested ? KIND_NESTED : 0) + (k.fast ? KIND_LIBRARY_TREE : 0) + (k.grouped ? KIND_GROUPED : 0) +
           (k.seg ? KIND_SEGMENTED : 0) + (adaptive ? KIND_ADAPTIVE : 0);
}

// a frame with light samples: the kind of the nested instantiation whose search it runs, and KIND_DIRECT
constexpr int film_direct_kind(const KernelProps &k, bool adaptive) { return kernel_kind(k, adaptive) | KIND_DIRECT; }

// ---- 2. The LDS layout of one instantiation for one scene ----
// Sizes of what the kernels keep in LDS besides the scene's tables (render.hip asserts that they are its own).
constexpr size_t kStagedNodeBytes = 72;                   // a reference-tree node row as staged (render.hip kLdsNodeBytes)
constexpr size_t kSurvivorQueueBytesPerWave = 16 * 64 * sizeof(uint16_t);  // sphere-list scan: kQueueCap entries per lane
constexpr size_t kParkedBytesPerThread = 12 * 8 + 5 * 4;  // five-wave instanced-list kernel (render.hip kParkBytesPerThread)
constexpr size_t kDefaultDynamicLds = 48 * 1024;          // what a launch may use without asking the runtime for more
struct LdsLayout {
    // byte offsets into the dynamic LDS block as in DeviceScene::lds_*; kNone = the kernel reads the global table
    uint32_t quad_aa = kNone, boxes = kNone, objects = kNone, xforms = kNone, media = kNone, materials = kNone, perlin = kNone,
             spheres_tab = kNone, group_boxes = kNone, mspheres = kNone, msphere_aux = kNone, sphere_aux = kNone;
    uint32_t fast_order = kNone, seg_media = kNone, seg_cand = kNone;
    uint32_t park = 0;
    uint32_t scan_pairs = kNone;
    uint32_t scan_spans = kNone;
    int lds_nodes = 0, lds_spheres = 0;  // RenderArgs::lds_nodes, ::lds_spheres
    size_t bytes = 0;                    // dynamic LDS of the launch (the render kernels have no static LDS)
    bool fits = true;                    // everything this instantiation reads from LDS only is staged
    // For rt_plan_launch (tests): what lies at the front of the block -- node rows, or survivor queues and sphere planes -- and
    // the unpadded size of every table this instantiation considered, staged or not, in the order of LdsTable.
    size_t front = 0;
    uint32_t table_bytes[RT_LDS_TABLES] = {};
};
// The slots of LdsLayout in the order rt_launch_plan lists them (include/rtow.h RT_LDS_TABLE_NAMES).
enum LdsTable : int {
    T_QUAD_AA, T_BOXES, T_OBJECTS, T_XFORMS, T_MEDIA, T_MATERIALS, T_PERLIN, T_SPHERES_TAB, T_GROUP_BOXES, T_MSPHERES, T_MSPHERE_AUX,
    T_SPHERE_AUX, T_FAST_ORDER, T_SEG_MEDIA, T_SEG_CAND, T_PARK, T_SCAN_PAIRS, T_SCAN_SPANS,
    kLdsTables,
};
static_assert(kLdsTables == RT_LDS_TABLES, "rt_launch_plan lists another number of tables than LdsLayout has slots");
// `sc`: only its count and flag fields are read (scene_counts)
LdsLayout lds_layout(const KernelProps &k, const DeviceScene &sc);
inline void apply_layout(const LdsLayout &l, DeviceScene &sc)
{
    sc.lds_quad_aa = l.quad_aa; sc.lds_boxes = l.boxes; sc.lds_objects = l.objects; sc.lds_xforms = l.xforms; sc.lds_media = l.media;
    sc.lds_materials = l.materials; sc.lds_perlin = l.perlin; sc.lds_spheres_tab = l.spheres_tab; sc.lds_group_boxes = l.group_boxes;
    sc.lds_mspheres = l.mspheres; sc.lds_msphere_aux = l.msphere_aux; sc.lds_sphere_aux = l.sphere_aux;
    sc.lds_fast_order = l.fast_order; sc.lds_seg_media = l.seg_media; sc.lds_seg_cand = l.seg_cand; sc.lds_park = l.park;
    sc.lds_scan_pairs = l.scan_pairs;
    sc.lds_scan_spans = l.scan_spans;
}

// ---- 3. The kernel choice ----
// The scene summary every decision reads: the count and flag fields of DeviceScene, filled from the flattened scene (no
// device needed; rt_scene_upload fills its tables' counts with the same function).  Every pointer is left alone.
void scene_counts(const FlatScene &f, DeviceScene &d);
struct KernelOptions {
    bool adaptive, force_general, always_walk, reference_tree, accelerate_lists;
    int pixels_per_wave;             // as settled by plan_frame (64 = one lane per ray)
    int width, rows_owned, num_cus;  // the film's share of the frame and the GPU's size
};
// BVH worlds without media are scanned, not walked, up to this many leaves and this scan cost (in half sphere tests,
// FlatScene::scan_cost)
constexpr uint32_t kSmallWorldLeaves = 16, kSmallWorldScanCost = 64;
KernelId choose_kernel(const DeviceScene &sc, const KernelOptions &o);

// ---- 4. The frame plan ----
struct FilmGeometry {
    int width, height, rows_owned;
    uint32_t n_pixels, n_tiles;  // pixels this rank owns, and their 8x8 tiles
};
FilmGeometry film_geometry(int width, int height, int stripe_rows, int rank, int world_size);
// Does every hit of a launch lie inside its leaf's box (variant: 0 strict, 1 fast)?  See launch_plan.cpp.
bool hits_stay_in_boxes(const FlatScene &f, const CameraRec &cam, int variant);
// Everything about a launch that does not depend on which grouped instantiation the final pixels_per_wave selects, from
// the kind and the LDS bytes of the kernel chosen for one lane per ray.
rt_launch_plan plan_frame(int kernel_kind, int lds_bytes, const FilmGeometry &film, int num_cus, const rt_render_params &p,
                          bool in_boxes, uint32_t n_world_nodes);
// The whole plan: kernel choice (with plan_frame's pixels_per_wave), LDS layout, frame plan.
rt_launch_plan plan_launch(const DeviceScene &sc, const FilmGeometry &film, int num_cus, const rt_render_params &p, bool adaptive,
                           bool in_boxes);

// ---- 5. The grid of a frame with light samples (render.hip film_direct_kernel) ----
// Persistent workgroups of 256 lanes that take pixels from a queue of n_tiles * 64 positions: as many as are resident at once
// -- `fit_per_cu` per CU as the runtime reports it (at least one), capped by max_blocks_per_cu where that is positive -- and
// never more than the queue has lanes' worth of positions; at least one.
uint32_t film_direct_blocks(int fit_per_cu, int max_blocks_per_cu, int num_cus, uint32_t n_tiles);

}  // namespace rtow
