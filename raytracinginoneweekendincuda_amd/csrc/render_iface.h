// render_iface.h -- launch interface between device_scene.cpp (host orchestration) and render.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adaptive_rule.h"
#include "flat_scene.h"
#include "rng.h"

namespace rtow {

struct SeedArgs {
    uint32_t *state;             // 6 planes of n_pixels words: d, v0..v4
    const uint32_t *jump_table;  // kJumpTableWords
    Xorwow base;                 // salted seed state (sequence 0)
    uint32_t *tile_cost;        // probe launches: rays traced per 8x8 tile (one counter per tile of this rank's rows)
    const uint32_t *tile_order; // render launches: queue position -> tile (nullptr = tiles in row-major order)
    int32_t probe;              // 1 = cost probe: trace `spp` samples per pixel, write nothing but tile_cost
    uint32_t n_pixels;
    int32_t width, stripe_rows, rank, world_size;
};

struct RenderArgs {
    double *pixels;              // rows_owned x width x 3
    double *accum;               // progressive rendering: running (unnormalised) colour sums, or nullptr
    int32_t spp_before;          // samples already in accum
    uint32_t *state;
    unsigned long long *ray_counter;
    uint32_t *cursor;            // pixel-queue cursor, zeroed before every launch
    uint32_t *tile_cost;        // probe launches: rays traced per 8x8 tile (one counter per tile of this rank's rows)
    const uint32_t *tile_order; // render launches: queue position -> tile (nullptr = tiles in row-major order)
    // The rehearsal (launch_plan.cpp plan_frame): the first `spp` samples of every pixel, their rays booked in tile_cost / pix_cost.
    // 1 = it writes nothing else (adaptive films: the frame launch renders every sample again); 2 = it keeps them: a pixel that
    // finishes saves its RNG words to `state` and its colour sum to `accum` (never `pixels`), and the frame launch resumes there.
    int32_t probe;
    // probe launches: a pixel whose rays reach this many books them and stops at once, in mid-sample, saving nothing (0 = no cap;
    // the pixel is on the longest-chain list whatever else it would have traced).  Its rays leave ray_counter again.
    int32_t probe_ray_cap;
    // frame launches behind a rehearsal that kept its samples: `spp` and `spp_before` are already moved by this many samples, and
    // a pixel whose pix_cost reached probe_ray_cap (it saved nothing) starts this many samples earlier, from its state as seeded
    int32_t resumed_spp;
    // Two classes of pixels (launch_plan.cpp plan_frame, device_scene.cpp enqueue_rehearsal): the probe books every pixel's rays in pix_cost;
    // classify_pixels marks the heavy ones in pix_class and lists them.  The render launch then serves both: the first
    // `heavy_waves` waves of every workgroup serve heavy_list (heavy_ppw pixels at a time, through heavy_cursor) and join
    // the tile queue when the list is done; the tile queue skips the pixels whose class is non-zero.
    uint32_t *pix_cost;               // probe launches: rays traced by each owned pixel (frame launches read it where resumed_spp and probe_ray_cap are set)
    const uint8_t *pix_class;         // tile queue: pixels whose class is non-zero are served from heavy_list / super_list
    const uint32_t *heavy_list;
    const uint32_t *heavy_count;
    // ... the very longest chains among them (classify_pixels: probed cost >= super_threshold) on a list of their own, which the
    // serving waves take from first, ONE pixel per wave and nothing beside it until it is done: the frame cannot end before that
    // pixel does, and alone in its wave its rays take two thirds of the time they take with five neighbours
    const uint32_t *super_list;
    const uint32_t *super_count;
    uint32_t *super_cursor;
    int32_t adaptive_ppw;             // fewer pixels per serving wave where the lists are short (render_kernel: fit)
    int32_t super_ppw;                // pixels of that list per serving wave (1 for BVH walks; sphere lists: 4, the grouped scan's 16 lanes per ray)
    uint32_t *heavy_cursor;
    int32_t heavy_waves, heavy_ppw, heavy_priority;
    uint32_t n_pixels;
    int32_t width, height, rows_owned;
    int32_t spp, max_depth;
    int32_t stripe_rows, rank, world_size;
    int32_t node_burst;     // composite BVH worlds: node visits between two leaf phases (set by the launcher)
    int32_t park_ratio;     // composite BVH worlds: the leaf phase starts once parked lanes outnumber moving ones by this factor
    int32_t leaf_batch;     // composite BVH worlds: a kind of leaf is tested once this many lanes of the wave wait for it
    int32_t rounds;         // kind-batched kernels: node / leaf rounds per look at the shading queue
    int32_t object_batch;   // the same for instances / groups (their cooperative scan serves one ray at a time: a small batch is fine)
    int32_t lds_nodes;      // set by the launcher (launch_plan.h lds_layout): BVH nodes are staged in LDS
    int32_t small_world;    // BVH worlds without media are scanned, not walked, up to this scan cost (and 16 leaves)
    int32_t accelerate_lists;  // list worlds of primitives: walk the library's tree instead of scanning the list
    int32_t exact_scan;     // sphere-list worlds: no conservative filter in front of the reference's sphere test
    int32_t filter_fp64;    // sphere-list worlds: the fp64 form of that filter, one sphere at a time (default: packed fp32, two at a time)
    int32_t reference_tree; // primitive BVH worlds: walk the reference's own tree in its own order (default: the library's SAH tree)
    int32_t always_walk;    // BVH worlds: walk the tree even where a scan of all leaves would be used (small scenes)
    int32_t force_general;  // tests: use the general kernel even where a specialised one applies
    int32_t coop_threshold; // sphere-list kernel: below this many live lanes a wave scans cooperatively
    int32_t coop_single;    // experiments: cooperative scan one ray at a time (the older scheme) instead of in groups
    int32_t num_cus;
    int32_t lds_spheres;    // set by the launcher (lds_layout): sphere planes staged in LDS for the cooperative scan
    int32_t overdue_priority;
    int32_t boost_rounds;   // overdue-only cooperative passes inserted after each pixel-parallel pass
    int32_t max_blocks_per_cu;  // cap on resident workgroups per CU (0 = whatever fits)
    int32_t pixels_per_wave;    // sphere-list kernel: at most this many lanes of a wave hold a pixel (64 = all of them)
    int32_t shade_batch;    // BVH kernels: shade once this many lanes have finished their walk
    uint32_t ray_budget;    // sphere-list kernel: a pixel past this many rays is finished cooperatively
    // sphere-list kernel: per 8x8 tile of this rank's rows the spheres a camera ray of the tile can reach (primary_cull_rule.h:
    // kPrimaryListWords uint16 per tile, built by launch_primary_lists ahead of the launch), or nullptr: every ray is scanned
    const uint16_t *primary_lists;
    // Adaptive sampling (adaptive_rule.h; the Adaptive<> instantiations of render.hip, chosen by `adaptive`): spp is then the most
    // samples a pixel may take in this launch.  Per owned pixel: samples taken so far in this frame, the sum of y^2 over them, and
    // whether the rule has stopped the pixel (a later launch of the frame drops it from the queue untouched).  The launcher zeroes
    // the three planes where a frame begins.  Samples taken by the launch are summed into ray_counter[2].
    int32_t adaptive;
    AdaptiveRule rule;
    uint32_t *ad_n;
    double *ad_q;
    uint8_t *ad_mark;
    // sphere-list kernel: the scan's runs are windowed (scan_window_rule.h; the tables lie behind the scan segments, flat_scene.h
    // ScanWindowSeg).  0: every run is scanned whole (RT_FLAG_NO_SCAN_WINDOWS, or no run of the scene has a table)
    int32_t scan_windows;
};

struct KernelInfo {
    int vgprs, lds_bytes, kind;  // kind: launch_plan.h kernel_kind() = WORLD * 8 + MEDIA * 4 + COMPOSITE * 2 + RICH + the KIND_* bits
};

// `kernel`: the instantiation to run, a KernelId.  Which one, what it stages in LDS and how the frame is scheduled is decided
// in launch_plan.h and nowhere else: these entry points run what they are given (and refuse what does not fit).
hipError_t launch_seed_strict(const SeedArgs &a, hipStream_t stream);
hipError_t launch_seed_fast(const SeedArgs &a, hipStream_t stream);
hipError_t launch_render_strict(int kernel, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream);
hipError_t launch_render_fast(int kernel, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream);
hipError_t kernel_info_strict(int kernel, const DeviceScene &sc, const RenderArgs &a, KernelInfo *info);
hipError_t kernel_info_fast(int kernel, const DeviceScene &sc, const RenderArgs &a, KernelInfo *info);

// the stopping rule as the adaptive render kernels of that build compile it, on device arrays of `count` entries (tests)
hipError_t launch_adaptive_rule_strict(const AdaptiveRule &rule, uint32_t count, const uint32_t *n, const double *sums_rgbq,
                                       const double *sample_rgb, double *q_out, uint8_t *stops_out, hipStream_t stream);
hipError_t launch_adaptive_rule_fast(const AdaptiveRule &rule, uint32_t count, const uint32_t *n, const double *sums_rgbq,
                                     const double *sample_rgb, double *q_out, uint8_t *stops_out, hipStream_t stream);

// First-hit feature pass (rt_film_render_features; the RT_FEATURES objects of render.hip): one lane per owned pixel, the
// reference's tree or list in the reference's order through the same leaf tests and make_surface as the render kernels.  The
// pixel's stream is seeded in the kernel (curand_init(seed, pixelIndex, 0)): the film's saved state is neither read nor written.
struct FeatureArgs {
    double *albedo, *normal;     // rows_owned x width x 3 each, compact like RenderArgs::pixels
    double *depth;               // rows_owned x width
    const uint32_t *jump_table;  // kJumpTableWords
    Xorwow base;                 // salted seed state (sequence 0)
    uint32_t n_pixels;
    int32_t width, height;
    int32_t samples;             // 0: one ray through the pixel centre; N >= 1: N camera_ray samples, averaged
    int32_t stripe_rows, rank, world_size;
};
hipError_t launch_features_strict(const DeviceScene &sc, const FeatureArgs &a, hipStream_t stream);
hipError_t launch_features_fast(const DeviceScene &sc, const FeatureArgs &a, hipStream_t stream);

// Ray queries (rt_scene_intersect; the RT_QUERY objects of render.hip): one lane per caller-supplied ray, the reference's tree or
// list in the reference's order as in the feature pass, every table from global memory.  Ray k's stream is seeded in the kernel,
// curand_init(seed, k + first_sequence, 0), and only where the scene has media: nothing else draws.
struct QueryArgs {
    const double *origin, *direction;   // count x 3 each
    const double *time, *tmin, *tmax;   // count each, or nullptr: the scalars below
    double time_all, tmin_all, tmax_all;
    double *t, *normal, *uv, *albedo;   // outputs, each may be nullptr (rt_query_hits)
    int32_t *leaf;
    uint8_t *front_face, *material, *occluded;
    // BVH worlds: per node of the world's tree, the positions among the world's leaves (rt_scene_dump_leaves order) of a bottom
    // node's leaves a and b (FlatScene::node_leaf_pos)
    const uint32_t *node_leaf_pos;
    unsigned long long *hit_counter;    // one word, zeroed by the caller: rays that report a hit; nullptr: not counted
    const uint32_t *jump_table;         // kJumpTableWords
    Xorwow base;                        // salted seed state (sequence 0)
    uint64_t first_sequence;
    uint32_t count;
    int32_t mode;                       // 0 closest hit, 1 occlusion (only `occluded` is written)
};
struct QueryKernelInfo {
    int vgprs, scratch_bytes;
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_query_strict(const DeviceScene &sc, const QueryArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_query_fast(const DeviceScene &sc, const QueryArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);

// Radiance queries (rt_scene_radiance; the RT_RADIANCE objects of render.hip): one lane per caller-supplied ray, `samples` paths
// from it one after the other -- the search of the ray queries, then make_surface and shade as in render_kernel -- all from the
// ray's one stream: rng_in[6k..6k+5] = {d, v0..v4} where given, else curand_init(seed, k + first_sequence, 0) in the kernel.
struct RadianceArgs {
    const double *origin, *direction;   // count x 3 each
    const double *time;                 // count, or nullptr: time_all
    double time_all;
    const uint32_t *rng_in;             // count x 6, or nullptr: seeded from base
    double *radiance;                   // count x 3: (1 / samples) * (sum of the samples), linear; may be nullptr
    uint32_t *path_rays;                // count: world searches over all samples of the ray; may be nullptr
    uint32_t *rng_out;                  // count x 6: the stream after the last draw; may be nullptr, may be rng_in
    unsigned long long *ray_counter;    // one word, zeroed by the caller: the sum of path_rays; nullptr: not counted
    const uint32_t *jump_table;         // kJumpTableWords
    Xorwow base;                        // salted seed state (sequence 0)
    uint64_t first_sequence;
    uint32_t count;
    int32_t samples, max_depth;
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_radiance_strict(const DeviceScene &sc, const RadianceArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_radiance_fast(const DeviceScene &sc, const RadianceArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);

// Path steps (rt_scene_path_step; the RT_STEP objects of render.hip): one lane per caller-supplied ray, one iteration of the radiance
// kernel's loop -- one search, make_surface, shade -- and what a caller needs to continue the path: rt_path_step_out's arrays.
// Every output may be nullptr (not all), and may be the input array of the same meaning: a lane reads before it writes.
struct StepArgs {
    const double *origin, *direction;   // count x 3 each
    const double *time;                 // count, or nullptr: time_all
    double time_all;
    const uint32_t *rng_in;             // count x 6, or nullptr: seeded from base
    uint8_t *status;                    // count: 0 miss, 1 the path ends at this hit, 2 scattered
    double *emitted, *attenuation;      // count x 3 each
    double *origin_out, *direction_out; // count x 3 each: the scattered ray, or the input ray where status != 2
    double *time_out;                   // count
    double *t, *normal;                 // count, count x 3: as QueryArgs
    uint8_t *front_face, *material;     // count each: as QueryArgs
    uint32_t *rng_out;                  // count x 6: the stream after the step's last draw
    unsigned long long *scattered_counter;  // one word, zeroed by the caller: rays of status 2; nullptr: not counted
    const uint32_t *jump_table;         // kJumpTableWords
    Xorwow base;                        // salted seed state (sequence 0)
    uint64_t first_sequence;
    uint32_t count;
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_step_strict(const DeviceScene &sc, const StepArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_step_fast(const DeviceScene &sc, const StepArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);

// Path advances (rt_scene_path_advance; the RT_ADVANCE objects of render.hip and advance_pack.hip): three launches on one stream.
//   1. advance_kernel: one lane per input row, step_kernel's iteration for the rows below n = min(*count_in, capacity) that are
//      alive; an ended ray is folded into `radiance`, a scattered one (a survivor) stages its record at its own row of the staging
//      arrays; every row below `capacity` gets its flag in `survivor`, every workgroup its number of survivors in block_counts.
//   2. launch_advance_scan: one workgroup, the exclusive prefix of block_counts into block_offsets, the total into *count_out.
//   3. launch_advance_gather: one lane per row; survivor k of workgroup b goes to row block_offsets[b] + (survivors before it in
//      the workgroup) of every output asked for: input order is kept.
// No workgroup waits for another: the order between the three is the stream's.  A staging array whose output is not asked for is
// nullptr and neither written nor read.
struct AdvanceStage {
    double *origin, *direction, *time;   // capacity x 3, x 3, x 1
    uint32_t *rng_state;                 // capacity x 6
    double *throughput;                  // capacity x 3
    int32_t *ray_id;                     // capacity
    double *t, *normal;                  // capacity, capacity x 3
    uint8_t *front_face, *material;      // capacity each
};
struct AdvanceArgs {
    const double *origin, *direction;   // capacity x 3 each
    const double *time;                 // capacity, or nullptr: time_all
    double time_all;
    const uint32_t *rng_in;             // capacity x 6, or nullptr: seeded from base
    const double *throughput;           // capacity x 3, or nullptr: (1, 1, 1)
    const int32_t *ray_id;              // capacity, or nullptr: k
    const uint8_t *alive;               // capacity, or nullptr: all
    const uint32_t *count_in;           // one word, or nullptr: capacity
    double *radiance;                   // sources x 3, or nullptr: nothing is folded
    AdvanceStage stage;                 // the workspace's rows (launch 1 writes, launch 3 reads)
    uint8_t *survivor;                  // capacity: 1 where row k scattered
    uint32_t *block_counts;             // one per workgroup of 256 rows
    unsigned long long *stepped_counter;  // one word, zeroed by the caller: rows stepped; nullptr: not counted
    const uint32_t *jump_table;         // kJumpTableWords
    Xorwow base;                        // salted seed state (sequence 0)
    uint64_t first_sequence;
    uint32_t capacity, sources;
};
struct AdvanceGatherArgs {
    AdvanceStage from, to;              // a nullptr in `to`: that output is not asked for
    const uint8_t *survivor;
    const uint32_t *block_offsets;
    uint32_t capacity;
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_advance_strict(const DeviceScene &sc, const AdvanceArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_advance_fast(const DeviceScene &sc, const AdvanceArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
// (advance_pack.hip: neither depends on the variant)
hipError_t launch_advance_scan(const uint32_t *block_counts, uint32_t *block_offsets, uint32_t n_blocks, uint32_t *count_out, hipStream_t stream);
hipError_t launch_advance_gather(const AdvanceGatherArgs &a, hipStream_t stream);
constexpr uint32_t kAdvanceBlock = 256;  // rows per workgroup of launches 1 and 3

// Path advances with light samples (rt_scene_path_advance_direct; the RT_ADVANCE_DIRECT objects of render.hip and advance_pack.hip):
// four launches on one stream.
//   1. advance_direct_kernel: advance_kernel's iteration, then, behind its reconvergence point, the light sample of the rows that
//      scattered from a diffuse or isotropic hit and one wave-uniform loop over the light table (staged in LDS as the light kernels
//      stage it) for the mixture density a lane needs: along its incoming ray where it ended on a lamp with a density carried in,
//      along its sample direction where it scattered.  A weighted lamp is folded here; a light sample that can add something
//      leaves its shadow ray, its weighted contribution and pending[k] = 1 at its row of the workspace.  stage.time and
//      stage.rng_state of `adv` are always given: launch 2 reads them.
//   2. shadow_kernel: one lane per row; a pending row searches the world as an occlusion query does, from the staged stream,
//      which it writes back where the scene has media, and adds its contribution to `radiance` where the lamp is visible.  A wave
//      without pending rows leaves at once.
//   3, 4. the scan and the gather of the plain advance; the gather moves scatter_pdf as well.
struct AdvanceDirectArgs {
    AdvanceArgs adv;
    const LightRow *rows;               // n_lights
    const double *cdf;                  // the cumulative table of the call's strategy, padded to an even length
    uint32_t n_lights;
    int32_t sample;                     // 1: draw a light sample at every diffuse or isotropic hit
    const double *scatter_pdf;          // capacity, or nullptr: all 0
    double *scatter_pdf_stage;          // capacity: the density the scattered ray was sent with, 0 where no sample was drawn
    double *shadow_direction, *shadow_distance, *shadow_radiance;  // capacity x 3, x 1, x 3: written where pending[k] is set
    uint8_t *pending;                   // capacity
    const uint32_t *node_leaf_pos;      // as QueryArgs
    unsigned long long *shadow_counters;  // two words, zeroed by the caller: shadow rays cast, shadow rays that reached their lamp; nullptr: not counted
};
struct AdvanceDirectGatherArgs {
    AdvanceGatherArgs rows;
    const double *scatter_pdf_from;
    double *scatter_pdf_to;             // nullptr: not asked for
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_advance_direct_strict(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_advance_direct_fast(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_advance_shadow_strict(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_advance_shadow_fast(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_advance_direct_gather(const AdvanceDirectGatherArgs &a, hipStream_t stream);

// Radiance queries with light samples (rt_scene_radiance_direct; the RT_RADIANCE_DIRECT objects of render.hip): the estimator of
// max_depth advances with light samples in one launch.  radiance_kernel's lane per ray and flattened loop, with one world search
// an iteration: of the lane's path ray, or of the shadow ray its last bounce left pending.  The light table comes as it comes to
// advance_direct_kernel and is staged in LDS the same way; there is no workspace.
struct RadianceDirectArgs {
    RadianceArgs rad;                   // rad.ray_counter counts path searches only
    const LightRow *rows;               // n_lights
    const double *cdf;                  // the cumulative table of the call's strategy, padded to an even length
    uint32_t n_lights;
    const uint32_t *node_leaf_pos;      // as QueryArgs
    unsigned long long *shadow_counters;  // two words, zeroed by the caller: shadow rays cast, shadow rays that reached their lamp; given where rad.ray_counter is
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_radiance_direct_strict(const DeviceScene &sc, const RadianceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_radiance_direct_fast(const DeviceScene &sc, const RadianceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);

// Frames with light samples (rt_render_launch_direct; the RT_FILM_DIRECT objects of render.hip): the film's planes as RenderArgs
// carries them, the light table and node_leaf_pos as RadianceDirectArgs carries them.  film_direct_kernel is
// radiance_direct_kernel's loop in persistent workgroups of 256 whose lanes take pixels from the queue word `cursor`, one
// wave-aggregated atomic a take; no rehearsal, no pixel classes, no tile order, no primary lists.
struct FilmDirectArgs {
    double *pixels;              // rows_owned x width x 3
    double *accum;               // progressive rendering: running (unnormalised) colour sums, or nullptr
    int32_t spp_before;          // samples already in accum
    uint32_t *state;             // 6 planes of n_pixels words: d, v0..v4
    unsigned long long *ray_counter;  // [0] path searches, [2] samples taken (adaptive sampling), as RenderArgs
    uint32_t *cursor;            // pixel-queue cursor, zeroed before every launch
    uint32_t n_pixels;
    int32_t width, height, rows_owned;
    int32_t spp, max_depth;
    int32_t stripe_rows, rank, world_size;
    int32_t num_cus;
    int32_t max_blocks_per_cu;   // cap on resident workgroups per CU (0 = whatever fits)
    int32_t adaptive;            // as RenderArgs: spp is the most a pixel may take in this launch
    AdaptiveRule rule;
    uint32_t *ad_n;
    double *ad_q;
    uint8_t *ad_mark;
    const LightRow *rows;               // n_lights
    const double *cdf;                  // the cumulative table of the launch's strategy, padded to an even length
    uint32_t n_lights;
    const uint32_t *node_leaf_pos;      // as QueryArgs
    unsigned long long *shadow_counters;  // two words, zeroed by the caller: shadow rays cast, shadow rays that reached their lamp
};
struct FilmDirectInfo {
    KernelInfo kernel;  // kind: the nested instantiation's, with KIND_DIRECT
    int scratch_bytes;
};
// info != nullptr: report the instantiation that would run instead of launching it
hipError_t launch_film_direct_strict(const DeviceScene &sc, const FilmDirectArgs &a, hipStream_t stream, FilmDirectInfo *info = nullptr);
hipError_t launch_film_direct_fast(const DeviceScene &sc, const FilmDirectArgs &a, hipStream_t stream, FilmDirectInfo *info = nullptr);

// Light sampling queries (rt_scene_sample_lights, rt_scene_light_pdf; the RT_LIGHTS objects of render.hip): one lane per point or
// ray, 256-thread workgroups that first stage the first kLightLdsRows rows of the light table and of its cumulative table in LDS.
// The table is not part of DeviceScene: it comes through these arguments.  `sc` is still passed, for the material and texture
// tables that `emitted` reads.
struct LightArgs {
    const LightRow *rows;               // n_lights
    const double *cdf;                  // the cumulative table of the call's strategy, padded to an even length
    uint32_t n_lights;
    // mode 0 (light_sample_kernel): points in, samples out; mode 1 (light_pdf_kernel): origin = point, direction in, pdf / light out
    const double *point;                // count x 3
    const double *direction_in;         // count x 3 (mode 1)
    const double *normal;               // count x 3, or nullptr
    const uint8_t *material;            // count, or nullptr
    const double *time;                 // count, or nullptr: time_all
    double time_all;
    const uint32_t *rng_in;             // count x 6, or nullptr: seeded from base
    double *direction, *distance;       // outputs of mode 0, each may be nullptr
    int32_t *light;                     // count (both modes)
    double *pdf;                        // count (both modes)
    double *emitted, *scatter_pdf, *contribution;
    uint32_t *rng_out;                  // count x 6; may be rng_in
    unsigned long long *valid_counter;  // one word, zeroed by the caller: valid samples / rays that meet a light; nullptr: not counted
    const uint32_t *jump_table;         // kJumpTableWords
    Xorwow base;                        // salted seed state (sequence 0)
    uint64_t first_sequence;
    uint32_t count;
};
// info != nullptr: report the kernel that would run instead of launching it
hipError_t launch_light_sample_strict(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_light_sample_fast(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_light_pdf_strict(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_light_pdf_fast(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
// Environment sampling (rt_scene_sample_environment, rt_scene_environment_pdf; the same objects): the light calls' arguments
// without a table -- rows, cdf, n_lights, point and time stay unread; the tables are the EnvRec's behind the camera's record.
// `light` receives the texel, j * width + i, or -1 where the environment has no distribution.
hipError_t launch_env_sample_strict(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_env_sample_fast(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_env_pdf_strict(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);
hipError_t launch_env_pdf_fast(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info = nullptr);

// One level of the edge-avoiding a-trous filter (denoise.hip; include/rtow.h rt_denoise_params has the stencil): full-frame
// planes, `in` and `out` distinct.  A guide that is nullptr switches its term off; inv_* = 1 / sigma^2 (0 for sigma = +inf), the
// colour's already scaled for the level.
struct AtrousArgs {
    const double *in;       // height x width x 3
    double *out;
    const double *albedo, *normal;  // height x width x 3, or nullptr
    const double *depth;            // height x width, or nullptr
    int32_t width, height, step;
    double inv_color, inv_albedo, inv_normal, inv_depth;
};
hipError_t launch_atrous(const AtrousArgs &a, hipStream_t stream);

// class 1 + an entry in `list` (its length in *count, which the caller has zeroed) for every pixel whose probed cost is at
// least `threshold` rays, class 0 for the others; with super_list: the pixels of at least super_threshold rays go there instead
// (length count[1])
hipError_t launch_classify_pixels(const uint32_t *pix_cost, uint32_t n_pixels, uint32_t threshold, uint8_t *pix_class, uint32_t *list,
                                  uint32_t *count, hipStream_t stream, uint32_t *super_list = nullptr, uint32_t super_threshold = 0,
                                  uint32_t width = 0, uint32_t near_percent = 0, uint32_t near_neighbours = 0);  // a pixel of near_percent % of the threshold with that many of its 8 neighbours over it is listed too

// lists[tile * kPrimaryListWords ..]: the list of primary_cull_rule.h for every 8x8 tile of the rank's rows (one thread per tile,
// the scene's static spheres on the scalar path); `sc.camera` and `sc.spheres` are the uploaded tables
hipError_t launch_primary_lists(const DeviceScene &sc, uint16_t *lists, uint32_t n_tiles, int32_t width, int32_t height, int32_t rows_owned,
                                int32_t stripe_rows, int32_t rank, int32_t world_size, hipStream_t stream);

// tile_order[k] = the tile with the k-th highest cost (counting sort over 256 cost classes; one workgroup)
// (flat_x8 / 8 = ratio of the heaviest tile to the mean below which the row-major order is kept)
hipError_t launch_tile_order(const uint32_t *tile_cost, uint32_t *tile_order, uint32_t n_tiles, uint32_t flat_x8, hipStream_t stream);

} // namespace rtow
