// launch_plan.cpp -- see launch_plan.h: the kernel choice, the LDS layout and the frame plan of a launch, host-only.
#include "launch_plan.h"

#include <cassert>
#include <cmath>
#include <cstring>

#include "scene_host.h"

namespace rtow {

// ---- the LDS layout -------------------------------------------------------------------------------------------------
// Budgets of the dynamic LDS block, each with its reason:
constexpr size_t kNodeRowsMost = 60 * 1024;      // node rows are staged up to here: keep >= 2 workgroups (of 256 threads) per CU resident
constexpr size_t kWholeCuBudget = 158 * 1024;    // one workgroup of 768 threads has (nearly) all of the CU's 160 KB
constexpr size_t kSharedCuBudget = 52 * 1024;    // three 256-thread workgroups per CU share its 160 KB
constexpr size_t kSpherePlanesMost = 48 * 1024;  // sphere-list worlds: the planes of the cooperative scan are staged up to here (behind the survivor queues), read from L2 beyond
constexpr size_t kPlaceSlack = 64;               // what a placed table leaves free of its budget

LdsLayout lds_layout(const KernelProps &k, const DeviceScene &sc)
{
    LdsLayout l;
    size_t lds = 0, off = 0, budget = 0;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    // a table goes behind what is placed already if it is not empty, within its own cap, and leaves the slack of the budget
    auto place = [&](LdsTable t, uint32_t &slot, size_t bytes, size_t cap) {
        l.table_bytes[t] = (uint32_t)bytes;
        if (bytes == 0 || bytes > cap || off + bytes + kPlaceSlack > budget) return;
        slot = (uint32_t)off;
        off += up16(bytes);
    };
    auto staged = [](uint32_t n, uint32_t slot) { return n == 0 || slot != kNone; };
    auto empty = [](uint32_t &slot) { if (slot == kNone) slot = 0; };  // an empty table is never read
    const bool big = k.block >= kBigBlockThreads;
    const size_t no_cap = ~(size_t)0;
    if (k.world == 0) {
        const size_t need = (k.fast || k.seg) ? (size_t)sc.n_fast_nodes * sizeof(FastNodeF) : (size_t)sc.n_world_nodes * kStagedNodeBytes;
        if (need <= kNodeRowsMost) {
            lds = need;
            l.lds_nodes = 1;
        }
        l.front = lds;
        if (k.fast && big) {
            // One workgroup per CU: the sphere rows the leaf tests and the hit record read and the material rows follow the
            // node rows into the CU's LDS -- a frame ends with its longest pixel, and that pixel's chain is made of exactly
            // these dependent reads (C3: leaf pass 2100 -> ... cycles, shading pass 11000 -> ... cycles).
            if (l.lds_nodes) {
                budget = kWholeCuBudget;
                off = up16(lds);
                place(T_MSPHERES, l.mspheres, (size_t)sc.n_mspheres * sizeof(MSphereGeom), no_cap);
                place(T_MSPHERE_AUX, l.msphere_aux, (size_t)sc.n_mspheres * sizeof(SphereAux), no_cap);
                place(T_SPHERES_TAB, l.spheres_tab, (size_t)sc.n_spheres * sizeof(SphereGeom), no_cap);
                place(T_SPHERE_AUX, l.sphere_aux, (size_t)sc.n_spheres * sizeof(SphereAux), no_cap);
                place(T_MATERIALS, l.materials, (size_t)sc.n_materials * sizeof(MaterialRec), no_cap);
                lds = off;
            }
            // The library-tree kernel reads these rows from LDS only (no global side in its accessors: head of
            // render_kernel); a world whose rows do not fit is walked by the reference-tree kernel (choose_kernel).
            l.fits = l.lds_nodes && staged(sc.n_mspheres, l.mspheres) && staged(sc.n_mspheres, l.msphere_aux) &&
                     staged(sc.n_spheres, l.spheres_tab) && staged(sc.n_spheres, l.sphere_aux) && staged(sc.n_materials, l.materials);
            empty(l.mspheres); empty(l.msphere_aux); empty(l.spheres_tab); empty(l.sphere_aux); empty(l.materials);
        }
        if (k.seg) {  // the leaf positions per node and the media, right behind the node rows
            off = up16(lds);
            l.fast_order = (uint32_t)off;
            off += up16(l.table_bytes[T_FAST_ORDER] = (uint32_t)((size_t)sc.n_fast_nodes * sizeof(FastOrder)));
            l.seg_media = (uint32_t)off;
            off += up16(l.table_bytes[T_SEG_MEDIA] = (uint32_t)((size_t)(sc.n_seg_media ? sc.n_seg_media : 1u) * sizeof(SegMedium)));
            l.seg_cand = (uint32_t)off;
            off += up16(l.table_bytes[T_SEG_CAND] = (uint32_t)((size_t)(sc.n_seg_cand ? sc.n_seg_cand : 1u) * sizeof(SegCandidate)));
            lds = off;
        }
        if (k.composite) {
            // Small tables ride along behind the node rows, each on its own merits: the records a leaf test or the shading
            // chases through (object -> transforms -> medium; material rows; Perlin tables: a few KB even in the Book-2
            // final scene) and, where they fit as well, the quad / box rows (Cornell box: 2 KB).
            budget = big ? kWholeCuBudget : kSharedCuBudget;
            off = up16(lds);
            place(T_OBJECTS, l.objects, (size_t)sc.n_objects * sizeof(ObjectRec), 4096);
            place(T_XFORMS, l.xforms, (size_t)sc.n_xforms * sizeof(Xform), 4096);
            place(T_MEDIA, l.media, (size_t)sc.n_media * sizeof(MediumRec), 2048);
            place(T_GROUP_BOXES, l.group_boxes, (size_t)sc.n_group_boxes * sizeof(GroupBox), 4096);
            place(T_MATERIALS, l.materials, (size_t)sc.n_materials * sizeof(MaterialRec), 4096);
            if (k.rich) place(T_PERLIN, l.perlin, (size_t)sc.n_perlin * sizeof(PerlinRec), 2 * sizeof(PerlinRec));
            const size_t b_quads = (size_t)sc.n_quads * sizeof(AAQuad), b_boxes = (size_t)sc.n_boxes * sizeof(BoxRec);
            l.table_bytes[T_QUAD_AA] = (uint32_t)b_quads;  // (placed together or not at all where workgroups share the CU)
            l.table_bytes[T_BOXES] = (uint32_t)b_boxes;
            if (big) {  // the big tables, most useful first
                place(T_BOXES, l.boxes, b_boxes, 80 * 1024);
                place(T_SPHERES_TAB, l.spheres_tab, (size_t)sc.n_spheres * sizeof(SphereGeom), 40 * 1024);
                place(T_QUAD_AA, l.quad_aa, b_quads, 16 * 1024);
            } else if (b_quads + b_boxes <= 16 * 1024 && off + b_quads + b_boxes + 96 <= budget) {
                place(T_QUAD_AA, l.quad_aa, b_quads, 16 * 1024);
                place(T_BOXES, l.boxes, b_boxes, 16 * 1024);
            }
            lds = off;
            if (k.batch && big) {
                // The deep kernel reads its node rows and every table from LDS only (its accessors have no global side: see
                // the head of render_kernel).  A scene that does not fit goes to the general kernel, which reads what is
                // not staged from L2 (choose_kernel).
                l.fits = l.lds_nodes && staged(sc.n_objects, l.objects) && staged(sc.n_xforms, l.xforms) && staged(sc.n_media, l.media) &&
                         staged(sc.n_group_boxes, l.group_boxes) && staged(sc.n_materials, l.materials) && staged(sc.n_perlin, l.perlin) &&
                         staged(sc.n_boxes, l.boxes) && staged(sc.n_spheres, l.spheres_tab);
                // (the quad rows stay optional: a box's six faces are read only for a hit point on one of its edges)
                empty(l.objects); empty(l.xforms); empty(l.media); empty(l.group_boxes); empty(l.materials);
                empty(l.perlin); empty(l.boxes); empty(l.spheres_tab);
            }
        }
    } else if (k.world == 2) {
        lds = (size_t)(k.block / 64) * kSurvivorQueueBytesPerWave;
        const size_t planes = (size_t)((sc.n_spheres + 63u) & ~63u) * 5 * sizeof(double);
        if (planes <= kSpherePlanesMost) {
            lds += planes;
            l.lds_spheres = 1;
        }
        l.front = lds;
        // the grouped scan's packed fp32 rows (render.hip scan_grouped), 16 B a padded row in two planes of 16 B a pair, behind the fp64
        // planes: only with them, and only where the block stays within kSharedCuBudget -- the third workgroup per CU is worth more
        // than the filter (a block the planes alone carry past that budget would pass 64 KB with the rows)
        const size_t pair_rows = (size_t)((sc.n_spheres + 63u) & ~63u) * 2 * sizeof(float) * 2;
        if (l.lds_spheres && lds + pair_rows <= kSharedCuBudget) {
            l.scan_pairs = (uint32_t)lds;
            lds += pair_rows;
            l.table_bytes[T_SCAN_PAIRS] = (uint32_t)pair_rows;
        }
        // the window spans of the scan's trips (scan_window_rule.h; render.hip scan_filtered32 reads one per lane and chunk of 64 trips),
        // 8 B a trip, where some run of the scene has a table: with the planes, under the same budget (C2: 61 trips, 488 B)
        const size_t span_rows = (size_t)sc.n_scan_window_trips * 8;
        l.table_bytes[T_SCAN_SPANS] = (uint32_t)span_rows;
        if (l.lds_spheres && span_rows && up16(lds) + span_rows <= kSharedCuBudget) {
            l.scan_spans = (uint32_t)up16(lds);
            lds = up16(lds) + span_rows;
        }
    }
    if (k.park) {  // the parked path state, one entry per thread (list worlds stage no tables: their rows come through scalar loads)
        off = up16(lds);
        l.park = (uint32_t)off;
        lds = off + (l.table_bytes[T_PARK] = (uint32_t)((size_t)k.block * kParkedBytesPerThread));
    }
    l.bytes = lds;
    return l;
}

// ---- the kernel choice ----------------------------------------------------------------------------------------------
void scene_counts(const FlatScene &f, DeviceScene &d)
{
    d.world_kind = f.world_kind;
    d.n_world_items = (uint32_t)f.world_items.size();
    d.n_nodes = (uint32_t)f.nodes.size();
    d.n_world_nodes = f.n_world_nodes;
    d.scan_cost = f.scan_cost;
    d.n_spheres = (uint32_t)f.spheres.size();
    d.n_mspheres = (uint32_t)f.mspheres.size();
    d.n_quads = (uint32_t)f.quads.size();
    d.n_objects = (uint32_t)f.objects.size();
    d.n_boxes = (uint32_t)f.boxes.size();
    d.n_xforms = (uint32_t)f.xforms.size();
    d.ms_padded = f.ms_padded;
    d.n_fast_nodes = (uint32_t)f.fast_nodes.size();
    d.n_seg_media = (uint32_t)f.seg_media.size();
    d.n_seg_cand = (uint32_t)f.seg_cand.size();
    d.n_media = (uint32_t)f.media.size();
    d.n_materials = (uint32_t)f.materials.size();
    d.n_perlin = (uint32_t)f.perlin.size();
    d.n_group_boxes = (uint32_t)f.group_boxes.size();
    d.n_scan_segments = (uint32_t)f.scan_segments.size();
    d.n_scan_window_trips = (uint32_t)f.scan_trip_spans.size();
    d.flags = f.flags;
    apply_layout(LdsLayout{}, d);  // nothing is staged until a launch lays its LDS out
}

constexpr uint32_t kDeepWorldNodes = 64;  // a world BVH of more nodes is "deep": see plan_frame, choose_kernel

// Four or five waves per SIMD for the instanced-list kernel (TListInstances5): whole generations of pixels on the resident
// lanes times the duration of a pass at that occupancy (1 : 1.38, measured on C4: three generations of 85.7 ms against two of
// 118.6).  A frame that does not fill the lanes of four waves stays there: its time is its pixels' chains, and a pass is shortest
// with the fewest waves.
static int list_instances_waves(const KernelOptions &o)
{
    const double pixels = (double)o.width * (double)o.rows_owned;
    const double cus = o.num_cus > 0 ? (double)o.num_cus : 256.0;
    const double gen4 = std::ceil(pixels / (cus * 16.0 * 64.0) - 0.02), gen5 = std::ceil(pixels / (cus * 20.0 * 64.0) - 0.02);
    if (gen4 <= 1.0) return 4;
    return gen5 * 1.38 < gen4 ? 5 : 4;
}

KernelId choose_kernel(const DeviceScene &sc, const KernelOptions &o)
{
    const bool composite = sc.n_objects != 0 || sc.n_boxes != 0;
    // (an environment is read by the instantiations that carry the texture code: render.hip miss_value)
    const bool rich = (sc.flags & (SCENE_RICH_TEXTURES | SCENE_ENVIRONMENT)) != 0, media = (sc.flags & SCENE_HAS_MEDIA) != 0, trees = (sc.flags & SCENE_HAS_TREES) != 0;
    const bool library_tree = sc.n_fast_nodes != 0;
    // an instantiation that reads its tables from LDS only is chosen where they fit, and the next best one where they do not
    auto fits = [&](KernelId k) { return lds_layout(kKernelProps[k], sc).fits; };
    // RT_FLAG_ACCELERATE_LISTS: a list world of primitives through the library's tree, when its rows fit the kernel's LDS
    if (o.accelerate_lists && sc.world_kind == WORLD_LIST && library_tree && !composite && !rich && !media && !trees && !o.force_general &&
        fits(K_BVH_PRIMS_FAST))
        return K_BVH_PRIMS_FAST;
    if ((sc.flags & SCENE_LIST_ALL_SPHERES) && !rich && sc.n_spheres <= 65535u && !o.force_general) return K_SPHERE_LIST;
    if (trees) return sc.world_kind == WORLD_BVH ? K_BVH_NESTED : K_LIST_NESTED;
    // small BVH worlds are scanned like lists (render.hip, at the list instantiations): up to 16 leaves within a scan budget in
    // half sphere tests, see FlatScene::scan_cost
    const bool scan_world = sc.world_kind == WORLD_LIST ||
                            (sc.n_world_items <= kSmallWorldLeaves && sc.scan_cost <= kSmallWorldScanCost && !o.always_walk);
    if (scan_world && !rich && !media && !o.force_general) {
        // pixels_per_wave < 64 (a power of two: plan_frame): the instantiation that deals a ray's leaves to lanes
        const bool grouped = o.pixels_per_wave < 64 && (o.pixels_per_wave & (o.pixels_per_wave - 1)) == 0 && o.pixels_per_wave > 0;
        if (grouped) return composite ? K_LIST_INSTANCES_GROUPED : K_LIST_PRIMS_GROUPED;
        // Adaptive frames take the four-wave build: the five-wave one (Traits::PARK) is chosen where a frame is a whole number of
        // generations of pixels that all cost the same (list_instances_waves), which pixels that stop at different sample counts
        // no longer are -- and its parked state has no room for q without giving back the registers the parking won.
        if (composite && !o.adaptive && list_instances_waves(o) == 5) return K_LIST_INSTANCES_5;
        return composite ? K_LIST_INSTANCES : K_LIST_PRIMS;
    }
    if (sc.world_kind == WORLD_BVH) {
        if (!composite && !rich && !o.force_general)
            return library_tree && !o.reference_tree && fits(K_BVH_PRIMS_FAST) ? K_BVH_PRIMS_FAST : K_BVH_PRIMS;
        if (!rich && !o.force_general) return media ? K_BVH_MEDIA : K_BVH_INSTANCES;
        // deep worlds: the library's tree, one walk per run of surfaces between media, where the scene has one (RT_FLAG_REFERENCE_TREE:
        // the reference's tree in the reference's order); both fall back when their tables do not fit the LDS of a CU
        const bool deep = sc.n_world_nodes > kDeepWorldNodes;
        if (deep && (sc.flags & SCENE_SEGMENTED) && !o.reference_tree && library_tree && sc.n_seg_media <= kSegMaxMedia && fits(K_BVH_SEGMENTED))
            return K_BVH_SEGMENTED;
        return deep && fits(K_BVH_GENERAL_DEEP) ? K_BVH_GENERAL_DEEP : K_BVH_GENERAL;
    }
    return K_LIST_GENERAL;
}

// ---- the frame plan -------------------------------------------------------------------------------------------------
FilmGeometry film_geometry(int width, int height, int stripe_rows, int rank, int world_size)
{
    FilmGeometry g{};
    g.width = width;
    g.height = height;
    g.rows_owned = rt_stripe_rows(height, stripe_rows, rank, world_size, nullptr, 0);
    g.n_pixels = (uint32_t)g.rows_owned * (uint32_t)width;
    g.n_tiles = (((uint32_t)width + 7u) >> 3) * (((uint32_t)g.rows_owned + 7u) >> 3);
    return g;
}

// Does every hit of this launch lie inside its leaf's box?  The library's own search structures -- its SAH tree, the scan of
// all leaves of a small BVH world, the segmented walk, RT_FLAG_ACCELERATE_LISTS, the thin-wave scan -- meet the leaves in
// another order than the reference's tree, and find the reference's closest hit only because (1) no leaf they search draws
// random numbers and (2) no hit lies outside its leaf's box, where the reference's tree would cull it.  A moving sphere
// leaves its box (c0 .. c1) at ray times outside its own [time0, time1] (R/MovingSphere.h:51 does not clamp frac), so
// the camera's shutter decides, per launch.  The ray times are those of render.hip camera_ray, time0 + u * (time1 - time0),
// with u = xorwow_uniform in [2^-33, 1] (monotone in u; the fast build fuses the multiply-add); frac is (tm - t0) / dt as in
// msphere_center, which a unit-time row evaluates as tm itself -- the same value.
bool hits_stay_in_boxes(const FlatScene &f, const CameraRec &cam, int variant)
{
    if (f.ms_nonfinite) return false;
    if (f.ms_intervals.empty()) return true;
    const double span = cam.time1 - cam.time0;
    double tm[2];
    const double u[2] = {(double)0x1p-33f, 1.0};
    for (int k = 0; k < 2; k++) {
        if (variant) {
            tm[k] = std::fma(u[k], span, cam.time0);
        } else {
            volatile double prod = u[k] * span;  // no contraction: the strict build's two roundings
            tm[k] = cam.time0 + prod;
        }
    }
    for (const MsInterval &iv : f.ms_intervals)
        for (double t : tm) {
            const double frac = (t - iv.t0) / iv.dt;
            if (!(frac >= 0.0 && frac <= 1.0)) return false;  // (NaN too)
        }
    return true;
}

// The three flags of the kernel choice as a launch sees them: a launch whose hits may leave their boxes takes the reference's
// tree in the reference's order (hits_stay_in_boxes), whatever the caller's flags say.
struct TreeFlags {
    int reference_tree, always_walk, accelerate_lists;
};
static TreeFlags tree_flags(const rt_render_params &p, bool in_boxes)
{
    if (!in_boxes) return TreeFlags{1 /* no library tree, no segmented walk */, 1 /* no scan of a small BVH world's leaves */, 0};
    return TreeFlags{(p.flags & RT_FLAG_REFERENCE_TREE) ? 1 : 0, (p.flags & RT_FLAG_ALWAYS_WALK) ? 1 : 0, (p.flags & RT_FLAG_ACCELERATE_LISTS) ? 1 : 0};
}

rt_launch_plan plan_frame(int kind, int lds_bytes, const FilmGeometry &film, int num_cus, const rt_render_params &p, bool in_boxes,
                          uint32_t n_world_nodes)
{
    rt_launch_plan plan;
    std::memset(&plan, 0, sizeof plan);
    const int spp = p.samples_per_pixel;
    const TreeFlags tree = tree_flags(p, in_boxes);
    plan.reference_tree = tree.reference_tree;
    plan.always_walk = tree.always_walk;
    plan.accelerate_lists = tree.accelerate_lists;
    plan.coop_threshold = p.coop_threshold > 0 ? p.coop_threshold : 24;
    plan.shade_batch = p.shade_batch > 0 ? p.shade_batch : 16;
    // A deep world BVH over composite leaves (scene 9: 400 boxes, two media, an instanced cluster): a leaf phase costs
    // tens of node steps there, so it pays to wait until most walkers have parked.  A shallow one (Cornell box: 8
    // leaves) gains nothing from waiting.
    plan.node_burst = n_world_nodes > kDeepWorldNodes ? 24 : 8;
    plan.park_ratio = n_world_nodes > kDeepWorldNodes ? 4 : 1;
    plan.leaf_batch = 12;
    plan.object_batch = 4;
    plan.rounds = 4;
    {
        // Off by default: on the Book-1 scenes a cooperative ray costs ~10x a pixel-parallel one, and every budget
        // tried (3..16 rays/sample, 2..32 boost rounds) lost more in throughput than it won back in frame tail.
        double per_sample = p.overdue_rays_per_sample > 0 ? (double)p.overdue_rays_per_sample : 1.0e9;
        double budget = per_sample * (double)spp;
        plan.ray_budget = budget >= 4.0e9 ? 0xFFFFFFFFu : (uint32_t)budget;
        if (p.overdue_rays_per_sample < 0) plan.ray_budget = 0xFFFFFFFFu;  // negative: never
    }
    // BVH sphere worlds: thin waves may scan all leaves together instead of walking (scan_grouped_ms), but the planes
    // come from L2 and a chip full of thin waves scanning is bound by L2 bandwidth: measured slower than walking at every
    // threshold (C3: 1748 Msamples/s never, 1681 at 17, 1048 at 33).  Off unless asked for.
    const bool bvh_kernel = is_bvh_kernel(kind);
    if (bvh_kernel && (p.coop_threshold <= 0 || !in_boxes)) plan.coop_threshold = 0;
    // A pixel's samples are one sequential chain (one RNG stream), so a frame cannot end before its longest pixel does
    // (glass: up to max_depth rays per sample).  One rehearsal of the first samples of every pixel, their rays counted, serves
    // two schedulers (what becomes of the samples themselves: probe_keeps below):
    //  * BVH worlds, heaviest tiles first: the 8x8 tiles are ranked by rays traced and the pixel queue hands them out in
    //    that order (in row-major order C3's queue drained at 38 ms and the last wave left at 99 ms);
    //  * sphere-list and primitive-BVH worlds, heavy and light pixels: the few pixels with long chains (0.4 % of C2's
    //    trace more than 10 rays per sample, up to 41) are listed; two waves of every workgroup serve that list first, a
    //    few pixels at a time -- the lanes share each ray's scan (sphere list: a third of the latency per ray at 1.8x the
    //    work), or simply have the wave to themselves (BVH walk) -- and then join the tile queue, whose pixels skip the
    //    listed ones.  C2 took 367 ms where its throughput alone needs ~310.
    // Every pixel is still rendered exactly once from its own stream: the frame is the same bit for bit
    // (tests: ...tile_ranking..., ...heavy_and_light...; RT_FLAG_ROW_MAJOR_TILES / RT_FLAG_NO_PIXEL_CLASSES turn them off).
    const bool sphere_list_kernel = is_sphere_list_kernel(kind), prim_bvh_kernel = is_prim_bvh_kernel(kind);
    const bool list_scan_kernel = is_list_scan_kernel(kind);
    //  * list worlds too (r3): a frame is a few "generations" of pixels per lane (C4: 640 k pixels on 262 k lanes), and the last
    //    generation lasts as long as its longest pixel while ever fewer lanes are busy (C4: queue dry at 148 ms, last wave out
    //    at 261).  Heaviest tiles first makes the pixels that start last the cheap ones.
    const bool rank_tiles = (bvh_kernel || list_scan_kernel || sphere_list_kernel) && spp >= 32 && film.n_tiles >= 1024 &&
                            !(p.flags & RT_FLAG_ROW_MAJOR_TILES);
    // the deep general kernel (one 768-thread workgroup per CU, C5): its ray chains are the longest of all (a ray takes ~140 us
    // in a full wave), which decides the frame whenever a GPU holds few pixels per lane -- a small frame, or one rank's share
    const bool deep_kernel = is_deep_kernel(kind, lds_bytes);
    // (r3) Heavy and light pixels for this kernel too -- where the frame is a few generations of pixels on the GPU's lanes, i.e. a
    // rank's stripes of a split frame.  C5 at 200 spp, one rank of N rendered alone: 699 / 712 / 646 / 597 / 709 / 479 ms for
    // N = 2 / 3 / 4 / 6 / 8 / 16 without classes -- no scaling at all, every rank waits for its longest chains -- and
    // 737 / 566 / 447 / 395 / 368 / 302 ms with them (profiles/r03_c5_roles.txt; the 8-way figure 293 with the settings of the
    // second sweep there: ten of twelve waves serving 32 pixels each from 8 rays per sample -- most of the frame, in half-filled waves).  A whole frame (13 generations) is throughput
    // and loses by them (1030 -> 1400 ms and worse), as it did in r2 with other settings; so: up to seven generations (a 2-way
    // split, 672 -> 626 ms), in three bands of settings.
    const double generations = (double)film.n_pixels / ((double)num_cus * 12.0 * 64.0);
    const bool deep_roles = deep_kernel && generations <= 7.0;
    // Both classes are served inside ONE launch, by wave (RenderArgs::heavy_list).  The library-tree kernel, whose 768-thread
    // workgroup fills a CU: C3 2106 -> 2713 Msamples/s; the primitive-BVH kernel on the reference's tree (256-thread
    // workgroups) gained nothing from classes (C3 1672 -> 1100-1200 with the heavy pixels in a second launch) and has none.
    // Sphere-list worlds: serving the heavy pixels from two waves of every workgroup lets the launch keep three workgroups per
    // CU resident (a third wave per SIMD: +15 % in the steady state, which a frame whose end is set by its long pixels could
    // not use) -- C2 1479 (a second launch for the heavy pixels, two workgroups per CU) -> 1556 Msamples/s.
    const bool ppw_given = p.pixels_per_wave > 0 && p.pixels_per_wave < 64;
    const bool split = (sphere_list_kernel || is_library_tree_prim_kernel(kind) || deep_roles) && !(p.flags & RT_FLAG_NO_PIXEL_CLASSES) &&
                       spp >= 64 && film.n_pixels >= 65536u && !ppw_given;
    plan.rank_tiles = rank_tiles;
    plan.pixel_classes = split;

    // pixels_per_wave < 64 gives every ray several lanes: the sphere list deals a ray's spheres to the lanes of a group (its
    // heavy-pixel waves do that by themselves, above), the list-scan kernels a ray's leaves (render.hip scan_leaves_grouped).
    // 0 = the library's choice, and that is 64 for every frame size measured: a pixel's samples are one sequential chain, a
    // launch ends with its longest pixel, and the pass of a wave that holds a few rays takes as long as one that holds 64 --
    // 17.6 us on the Cornell box whether the film owns 640 k pixels or 5 k (1 / 128 of C4: 118 ms for every split from 1 / 8
    // on) -- while the grouped pass is LONGER, not shorter: the eight leaves of that world are three kinds of code, which a
    // group of lanes executes one after the other just as one lane does, plus the exchange (C4 / 8: 117 ms at 64 pixels per
    // wave, 182 at 32, 201 at 16, 324 at 8; profiles/r03_lanes_per_ray.txt).  The parameter stays for worlds of one kind of
    // leaf and for experiments; the frames are bit-identical either way.
    {
        int ppw = ppw_given ? p.pixels_per_wave : 64;
        if (list_scan_kernel) {  // the grouped leaf scan deals lanes in powers of two
            int pow2 = 1;
            while (pow2 * 2 <= ppw) pow2 *= 2;
            ppw = pow2;
        }
        plan.pixels_per_wave = ppw;
    }
    // Sphere-list worlds: two resident workgroups per CU beat three although three fit -- a third wave per SIMD
    // speeds the steady state up, but with fewer pixels per lane the frame tail grows by more (measured on C2).  (With pixel
    // classes: three, see above; the rehearsal keeps two.)
    plan.probe_max_blocks_per_cu = p.max_blocks_per_cu > 0 ? p.max_blocks_per_cu : (sphere_list_kernel ? 2 : 0);
    plan.max_blocks_per_cu = plan.probe_max_blocks_per_cu;

    if (rank_tiles || split) {
        // sphere-list frames of 400 samples and more rehearse 8: the heavy pixels are told apart more reliably (C2, three
        // interleaved pairs in one call: 1859-1893 with 4, 1908-1918 with 8; the primitive-BVH kernel is better off with 4)
        int probe_spp = split ? (spp >= 400 ? 8 : 4) : spp / 100;  // (r3: 8 for the BVH kernel too, with the settings below)
        probe_spp = probe_spp < 1 ? 1 : (probe_spp > 8 ? 8 : probe_spp);
        if (probe_spp > spp) probe_spp = spp;
        plan.probe_spp = probe_spp;
        // The rehearsal is the frame's first probe_spp samples: every pixel saves its stream and its colour sum where it finishes
        // them, and the frame launch renders the spp - probe_spp that are left (C2: 8 of 500 sample passes were rendered twice).
        // Not for adaptive films: the rule's sum of y^2 and its check points would have to run in the plain kernel that rehearses;
        // their rehearsal writes nothing but ray counts and the frame launch starts every pixel at its first sample.
        plan.probe_keeps = (kind & KIND_ADAPTIVE) ? 0 : 1;
        assert(probe_spp < spp);  // ranking needs 32 samples, classes 64, at most 8 are rehearsed: the frame launch is never empty
    }
    // the order is kept row-major only where the heaviest tile is within an eighth of the mean (r3: was x4, which sorted for
    // glass only; C3 +1.7 % with every spread sorted, C2 / C5 indifferent between 9 / 8 and 32 / 8, one call)
    if (rank_tiles) plan.tile_flatness_x8 = 9;
    if (split) {
        // Serving settings (r3; every number below is the mean of several frames per setting in one call on one GPU -- earlier sweeps
        // took the best of two runs and missed a bimodal default; profiles/r03_c2_serving_sweep.txt, r03_c3_serving_sweep.txt,
        // r03_rank_serving_sweep.txt, r03_c5_roles.txt).  What per-pixel stamps showed: a light
        // pixel just under the threshold runs at a light wave's 30-40 us per ray from the frame's first millisecond to its last,
        // a listed pixel at 7-10 us -- threshold, serving capacity and the longest listed chain have to be moved together.
        //   sphere lists (C2)      two tiers: from 12 rays per sample four pixels to a serving wave (16 lanes per ray), from 9 eight;
        //                          two serving waves of four per workgroup.  Eight to a wave for all: 188...246 ms by which wave
        //                          held the longest chains; one tier of four: 198.6 ms; two tiers: 190.5
        //   primitive BVH (C3)     from 9 rays per sample six to a serving wave, three serving waves of twelve, eight rehearsed
        //                          samples; from 30 rays per sample ONE to a wave (super_list): 162 -> 153 ms
        //   deep segmented (C5)    only for frames of at most seven generations of pixels per lane (deep_roles above), 32 to a
        //                          serving wave: 8 / 12 / 16 rays per sample and 10 / 6 / 4 serving waves of twelve for up to
        //                          2.2 / 5 / 7 generations
        // A frame of few generations of pixels per lane (a rank's stripes) keeps these thresholds -- lower ones helped three
        // ranks of eight and cost the rank with the longest chains a third -- and lets its serving waves take fewer pixels each
        // (adaptive_ppw below).
        const bool few_generations = generations <= 3.0;  // of pixels per resident lane (twelve waves per CU)
        const int heavy_rays_per_sample = deep_roles ? (generations <= 2.2 ? 8 : (generations <= 5.0 ? 12 : 16)) : 9;
        const int super_rays = deep_roles ? 0 : (sphere_list_kernel ? 12 : 30);
        plan.heavy_threshold = heavy_rays_per_sample * plan.probe_spp;
        plan.super_threshold = super_rays * plan.probe_spp;
        // (primitive BVH worlds: a pixel probed at 70 % of the threshold with three of its eight neighbours over it is listed too --
        // the last pixel of a C3 frame was a light one probed at 8.75 rays per sample in a patch of heavy ones, really costing 16:
        // 152.5 -> 147.8 ms, six frames per setting; sphere lists: no difference, left off)
        plan.near_percent = prim_bvh_kernel ? 70 : 0;
        plan.near_neighbours = prim_bvh_kernel ? 3 : 0;
        if (super_rays > 0) plan.super_ppw = sphere_list_kernel ? 4 : 1;
        if (sphere_list_kernel && p.max_blocks_per_cu <= 0) plan.max_blocks_per_cu = 3;
        plan.heavy_waves = deep_roles ? (generations <= 2.2 ? 10 : (generations <= 5.0 ? 6 : 4)) : (sphere_list_kernel ? 2 : 3);
        plan.heavy_ppw = deep_roles ? 32 : (sphere_list_kernel ? 8 : 6);
        plan.heavy_priority = sphere_list_kernel ? 3 : 0;  // the serving waves' rays are the frame's critical path
        // fewer pixels per serving wave than the tuned numbers where the light pixels are few -- up to three generations of
        // pixels per lane, i.e. a rank's stripes of a split frame: the light side is short there and a listed chain is
        // shortest with its wave to itself (slowest rank, C2 / 4: 132 -> 119 ms, / 8: 135 -> 97; C3 / 2: 153 -> 135, / 4:
        // 154 -> 124, / 8: 155 -> 122).  A full frame packs the serving waves as densely as tuned: the ones left over join
        // the light queue at once (C3, 4.9 generations: 152 against 159 ms).
        plan.adaptive_ppw = few_generations ? 1 : 0;
        // The rehearsal knows no classes yet: its launch ends on its longest pixels (glass: up to max_depth rays per sample, every
        // one of them a pass of its wave), a handful the whole chip waits for -- and what it rehearses them for is decided at
        // super_threshold rays.  There a pixel stops, in mid-sample; it keeps nothing, the frame launch renders all its samples
        // (0.1-0.4 % of the pixels).  Tiles that hold such pixels book less than they cost: the ranking may move, the frame cannot.
        plan.probe_ray_cap = plan.super_threshold;
    }
    return plan;
}

// The layout as rt_launch_plan lists it: the slots of LdsLayout in the order of LdsTable, nothing decided or computed here.
static void show_layout(const LdsLayout &l, rt_launch_plan &plan)
{
    const uint32_t offsets[kLdsTables] = {l.quad_aa, l.boxes, l.objects, l.xforms, l.media, l.materials, l.perlin, l.spheres_tab,
                                          l.group_boxes, l.mspheres, l.msphere_aux, l.sphere_aux, l.fast_order, l.seg_media, l.seg_cand, l.park,
                                          l.scan_pairs, l.scan_spans};
    plan.lds_front_bytes = (int)l.front;
    for (int t = 0; t < kLdsTables; t++) {
        plan.lds_table_offset[t] = offsets[t];
        plan.lds_table_bytes[t] = l.table_bytes[t];
    }
}

rt_launch_plan plan_launch(const DeviceScene &sc, const FilmGeometry &film, int num_cus, const rt_render_params &p, bool adaptive,
                           bool in_boxes)
{
    // The kind depends on pixels_per_wave (the grouped instantiations), whose rounding depends on the kind: the frame is
    // planned from the kernel that one lane per ray selects, and pixels_per_wave then only picks that kernel's grouped form.
    KernelOptions o{};
    o.adaptive = adaptive;
    o.force_general = (p.flags & RT_FLAG_FORCE_GENERAL) != 0;
    const TreeFlags tree = tree_flags(p, in_boxes);
    o.always_walk = tree.always_walk != 0;
    o.reference_tree = tree.reference_tree != 0;
    o.accelerate_lists = tree.accelerate_lists != 0;
    o.pixels_per_wave = 64;
    o.width = film.width;
    o.rows_owned = film.rows_owned;
    o.num_cus = num_cus;
    const KernelId full = choose_kernel(sc, o);
    rt_launch_plan plan = plan_frame(kernel_kind(kKernelProps[full], adaptive), (int)lds_layout(kKernelProps[full], sc).bytes, film, num_cus,
                                     p, in_boxes, sc.n_world_nodes);
    o.pixels_per_wave = plan.pixels_per_wave;
    const KernelId kernel = choose_kernel(sc, o);
    const LdsLayout layout = lds_layout(kKernelProps[kernel], sc);
    plan.kernel = kernel;
    plan.kernel_kind = kernel_kind(kKernelProps[kernel], adaptive);
    plan.waves_per_simd = kKernelProps[kernel].min_waves;
    plan.lds_bytes = (int)layout.bytes;
    plan.lds_nodes = layout.lds_nodes;
    plan.lds_spheres = layout.lds_spheres;
    show_layout(layout, plan);
    o.adaptive = false;  // the rehearsal is the plain kernel's (of an adaptive film it only counts rays: probe_keeps)
    plan.probe_kernel = choose_kernel(sc, o);
    return plan;
}

uint32_t film_direct_blocks(int fit_per_cu, int max_blocks_per_cu, int num_cus, uint32_t n_tiles)
{
    uint32_t per_cu = fit_per_cu > 0 ? (uint32_t)fit_per_cu : 1u;
    if (max_blocks_per_cu > 0 && per_cu > (uint32_t)max_blocks_per_cu) per_cu = (uint32_t)max_blocks_per_cu;
    const uint32_t resident = per_cu * (uint32_t)(num_cus > 0 ? num_cus : 256);
    const uint32_t needed = (n_tiles + 3u) / 4u;  // a workgroup's 256 lanes are four tiles' positions
    const uint32_t blocks = needed < resident ? needed : resident;
    return blocks > 0 ? blocks : 1u;
}

}  // namespace rtow

using namespace rtow;

extern "C" int rt_plan_launch(rt_scene *scene, const rt_render_params *p, int num_cus, int adaptive, rt_launch_plan *out)
{
    if (!scene || !p || !out) return fail(RT_ERR_INVALID, "rt_plan_launch: null argument");
    const SceneImpl &s = *reinterpret_cast<SceneImpl *>(scene);
    if (!s.committed) return fail(RT_ERR_STATE, "rt_plan_launch: scene not committed (rt_scene_commit)");
    if (p->width <= 0 || p->height <= 0 || p->stripe_rows <= 0 || p->world_size <= 0 || p->rank < 0 || p->rank >= p->world_size || num_cus <= 0)
        return fail(RT_ERR_INVALID, "rt_plan_launch: bad geometry");
    if (p->samples_per_pixel < 0 || (p->variant != 0 && p->variant != 1) || p->pixels_per_wave < 0 || p->pixels_per_wave > 64)
        return fail(RT_ERR_INVALID, "rt_plan_launch: params rt_render_launch would refuse");
    DeviceScene counts{};
    scene_counts(s.flat, counts);
    *out = plan_launch(counts, film_geometry(p->width, p->height, p->stripe_rows, p->rank, p->world_size), num_cus, *p, adaptive != 0,
                       hits_stay_in_boxes(s.flat, s.camera, p->variant));
    return RT_OK;
}
