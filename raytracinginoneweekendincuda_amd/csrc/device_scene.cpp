// device_scene.cpp -- HIP side of the render API (include/rtow.h): table upload, the film (framebuffer +
// per-pixel RNG state, the reference's frameBuffer / randState, R/kernel.cu:606-613), launches and
// timing.  Replaces the host driver section R/kernel.cu:675-691.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rtow.h"
#include "device_arena.h"
#include "film_rows.h"
#include "launch_plan.h"
#include "primary_cull_rule.h"
#include "render_iface.h"
#include "scene_host.h"

namespace rtow {

static int hip_fail(hipError_t e, const char *what)
{
    return fail(RT_ERR_HIP, std::string("HIP error = ") + std::to_string((unsigned)e) + " (" + hipGetErrorString(e) +
                                ") at '" + what + "'");
}
#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

struct DeviceTables {
    uint64_t generation = 0;  // SceneImpl::generation these tables were made from
    DeviceArena memory;       // every table below
    DeviceScene scene{};
    const uint32_t *node_leaf_pos = nullptr;  // ray queries (rt_scene_intersect_device): FlatScene::node_leaf_pos
    bool scan_windows = false;  // sphere-list frames: some run of the scan has a window table (FlatScene::scan_windows)
    // light sampling queries (rt_scene_sample_lights_device): FlatScene::lights and its two cumulative tables
    const LightRow *lights = nullptr;
    const double *light_cdf[2] = {nullptr, nullptr};
    uint32_t n_lights = 0;
    // path advances without statistics return before their kernels have run (rt_scene_path_advance_device): recorded behind the
    // last of them, created by the first
    hipEvent_t advance_done = nullptr;
};

void release_device_tables(DeviceTables *t)
{
    if (t && t->advance_done) {  // an advance may still be reading the tables
        hipEventSynchronize(t->advance_done);
        hipEventDestroy(t->advance_done);
    }
    delete t;
}

// jump table: one copy per device for the life of the process
static std::mutex g_jump_mutex;
static std::map<int, uint32_t *> g_jump_tables;
static int device_jump_table(int device, const uint32_t **out)
{
    std::lock_guard<std::mutex> lock(g_jump_mutex);
    auto it = g_jump_tables.find(device);
    if (it == g_jump_tables.end()) {
        uint32_t *p = nullptr;
        HIP_TRY(hipMalloc((void **)&p, kJumpTableWords * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(p, host_jump_table(), kJumpTableWords * sizeof(uint32_t), hipMemcpyHostToDevice));
        it = g_jump_tables.emplace(device, p).first;
    }
    *out = it->second;
    return RT_OK;
}

static int select_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(RT_ERR_NO_DEVICE, "no HIP device available: the gfx950 render path cannot run (there is no CPU fallback)");
    if (device < 0 || device >= count) return fail(RT_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

constexpr size_t kCounterWords = 128;
constexpr size_t kHeavyCountWords = 16;  // FilmImpl::heavy_count: [0] length of heavy_list, [1] of super_list

struct FilmImpl {
    int device = 0;
    int stripe_rows = 8, rank = 0, world_size = 1;
    FilmGeometry geometry{};       // the frame's size and this rank's share of it (film_geometry)
    DeviceArena planes;            // every device pointer below that is the film's own, allocated at creation or on first use
    size_t plane_pixels() const { return geometry.n_pixels ? geometry.n_pixels : 1; }  // never an empty plane
    double *pixels = nullptr;      // where the kernel writes (own_pixels or a bound external buffer)
    double *own_pixels = nullptr;
    double *accum = nullptr;       // progressive rendering: unnormalised colour sums (allocated on first use)
    int accum_spp = 0;
    double *carry = nullptr;       // frames without RT_FLAG_ACCUMULATE: the sums a rehearsal hands to its frame launch (allocated on first use)
    uint32_t *state = nullptr;
    unsigned long long *ray_counter = nullptr;  // [0] rays, [2] samples taken (adaptive sampling), [1] / [6] / [9] low words = tile / heavy / super queue cursors, [7] and [32..119] phase sums
    int num_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t last_stream = nullptr;
    uint32_t *tile_cost = nullptr, *tile_order = nullptr;  // per 8x8 tile of this rank's rows: probed rays, and the tiles ranked by them
    // heavy / light pixels (allocated on first use): probed rays per pixel, the heavy pixels' list and count, every pixel's
    // class; the serving waves of the render launch take the listed pixels, the others the rest of the tile queue
    uint32_t *pix_cost = nullptr, *heavy_list = nullptr, *heavy_count = nullptr, *super_list = nullptr;  // heavy_count[1]: length of super_list
    uint8_t *pix_class = nullptr;
    uint16_t *primary_lists = nullptr;  // sphere-list worlds: the camera rays' candidates per tile (primary_cull_rule.h), rebuilt by every launch that reads them
    unsigned long long *host_counters = nullptr;  // pinned mirror of ray_counter, filled by an async copy behind the render
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // begin, after seed, after render, after the counter copy
    bool seeded = false;
    bool in_flight = false;
    SceneImpl *scene_in_flight = nullptr;  // the scene whose tables the launch in flight reads
    uint64_t last_samples = 0;
    int last_variant = 0;
    rt_launch_plan last_plan{};  // of the last launch
    KernelInfo last_kernel{};    // what launch_one reports of the kernel it was given (rt_render_stats)
    // adaptive sampling (rt_film_set_adaptive; adaptive_rule.h): the setting for the next launch, the setting the accumulated
    // frame in progress was begun with, and the per-pixel planes (allocated on first use): samples so far, sum of y^2, stopped
    bool adaptive = false, frame_adaptive = false, last_adaptive = false;
    AdaptiveRule rule{}, frame_rule{};
    uint32_t *ad_n = nullptr;
    double *ad_q = nullptr;
    uint8_t *ad_mark = nullptr;
    bool rendered = false;
    int frame_spp = 0;  // without adaptive: samples every owned pixel has had in the frame the film holds
    // first-hit feature planes (rt_film_render_features) and the filtered frame (rt_film_denoise), allocated on first use: compact
    // like the pixels; denoise_tmp is the other half of the filter's ping-pong
    double *feat_albedo = nullptr, *feat_normal = nullptr, *feat_depth = nullptr, *denoised = nullptr, *denoise_tmp = nullptr;
    bool has_features = false, has_denoised = false;
    // frames with light samples (rt_render_launch_direct): was the launch in flight (or the last one) a direct one, the private
    // memory of its kernel, and the statistics of the last one that rt_render_finish ended
    bool last_direct = false, has_direct_stats = false;
    int last_direct_scratch = 0;
    rt_film_direct_stats direct_stats{};
};
constexpr size_t kShadowCounterWord = 10;  // FilmImpl::ray_counter[10], [11]: shadow rays cast, shadow rays that reached their lamp (direct launches)

static bool same_rule(const AdaptiveRule &a, const AdaptiveRule &b)
{
    return a.min_samples == b.min_samples && a.check_interval == b.check_interval && a.noise_threshold == b.noise_threshold &&
           a.luminance_floor == b.luminance_floor;
}

static bool rule_in_range(const rt_adaptive_params &p)
{
    return p.min_samples >= 2 && p.check_interval >= 1 && p.noise_threshold >= 0.0 && std::isfinite(p.noise_threshold) &&
           p.luminance_floor > 0.0 && std::isfinite(p.luminance_floor);  // (comparisons with a NaN are false)
}
static AdaptiveRule to_rule(const rt_adaptive_params &p) { return AdaptiveRule{p.min_samples, p.check_interval, p.noise_threshold, p.luminance_floor}; }

// Does this launch add to the accumulated frame the film holds (as opposed to beginning a frame)?
static bool continues_frame(const FilmImpl &f, const rt_render_params *p)
{
    return (p->flags & RT_FLAG_ACCUMULATE) && (p->flags & RT_FLAG_KEEP_RNG_STATE) && f.seeded && f.accum && f.accum_spp > 0;
}

// A compact device plane of the film, `channels` values per pixel -> the full frame on the host.  The rows of other ranks
// are zeroed, as include/rtow.h documents for every download but rt_film_download, which leaves them as the caller had them.
template <class T>
static int download_rows(const FilmImpl &f, const T *device_plane, int channels, bool clear_other_rows, T *full)
{
    std::vector<T> compact((size_t)f.geometry.n_pixels * channels);
    if (f.geometry.n_pixels) HIP_TRY(hipMemcpy(compact.data(), device_plane, compact.size() * sizeof(T), hipMemcpyDeviceToHost));
    scatter_owned_rows(compact.data(), channels, f.geometry.width, f.geometry.height, f.stripe_rows, f.rank, f.world_size, clear_other_rows, full);
    return RT_OK;
}

// a launch of `s` into `f` is (about to be) in flight / is over
static void mark_in_flight(SceneImpl &s, FilmImpl &f)
{
    f.in_flight = true;
    f.scene_in_flight = &s;
    s.launches_in_flight++;
    s.films_in_flight.push_back(&f);
}
static void mark_done(FilmImpl &f)
{
    f.in_flight = false;
    if (SceneImpl *s = f.scene_in_flight) {
        s->launches_in_flight--;
        for (size_t k = 0; k < s->films_in_flight.size(); k++)
            if (s->films_in_flight[k] == &f) {
                s->films_in_flight.erase(s->films_in_flight.begin() + (long)k);
                break;
            }
        f.scene_in_flight = nullptr;
    }
}

void wait_for_films_in_flight(SceneImpl &s)
{
    int prev = 0;
    hipGetDevice(&prev);
    for (void *p : s.films_in_flight) {
        FilmImpl *f = static_cast<FilmImpl *>(p);
        hipSetDevice(f->device);
        // the whole stream, not only the last event: a launch that failed half-way has recorded no event
        if (f->last_stream) hipStreamSynchronize(f->last_stream);
        else if (f->ev[3]) hipEventSynchronize(f->ev[3]);
        f->scene_in_flight = nullptr;  // the film stays "in flight" until its rt_render_finish, which then only reports
    }
    hipSetDevice(prev);
    s.films_in_flight.clear();
    s.launches_in_flight = 0;
}

} // namespace rtow

using namespace rtow;

static inline SceneImpl *S(rt_scene *s) { return reinterpret_cast<SceneImpl *>(s); }
static inline FilmImpl *F(rt_film *f) { return reinterpret_cast<FilmImpl *>(f); }

// ---- lane-per-ray batches: what the eight families of calls on caller-supplied rays below share ----
// (ray queries, radiance, path steps, light samples, light densities, path advances, and the advances and the radiance with light
// samples: each a call on device arrays, which checks, fills its kernel's arguments and runs them, and a call on host arrays)
static const char *nothing_more() { return nullptr; }  // a family without a refusal of its own at one of batch_check's hooks
static const char *strategy_error(int32_t strategy)
{
    return strategy != 0 && strategy != 1 ? ": strategy must be 0 (uniform) or 1 (by area and brightness)" : nullptr;
}
// the per-ray input a batch cannot do without: a ray, or the point of a light sample
template <class Rays>
static const char *missing_input(const Rays *rays) { return !rays->origin || !rays->direction ? ": null origin or direction" : nullptr; }
static const char *missing_input(const rt_light_points *pts) { return !pts->point ? ": null point" : nullptr; }

// everything the families refuse alike without a device, in the order include/rtow.h lists it; `own` answers between the count and
// the variant, `after` behind the variant, with the family's refusal of its own parameters (": what is wrong") or nullptr
template <class Params, class Rays, class Own, class After = const char *(*)()>
static int batch_check(rt_scene *scene, const Params *p, const Rays *rays, const void *outputs, const std::string &name, Own own,
                       After after = nothing_more)
{
    if (!scene || !p || !rays || !outputs) return fail(RT_ERR_INVALID, name + ": null argument");
    if (!S(scene)->committed) return fail(RT_ERR_STATE, name + ": scene not committed (rt_scene_commit)");
    if (p->count < 0 || p->count > ((int64_t)1 << 30)) return fail(RT_ERR_INVALID, name + ": count must be 0 .. 2^30");
    if (const char *why = own()) return fail(RT_ERR_INVALID, name + why);
    if (p->variant != 0 && p->variant != 1) return fail(RT_ERR_INVALID, name + ": variant must be 0 (strict) or 1 (fast)");
    if (const char *why = after()) return fail(RT_ERR_INVALID, name + why);
    if (const char *why = p->count > 0 ? missing_input(rays) : nullptr) return fail(RT_ERR_INVALID, name + why);
    return RT_OK;
}

// What a call with statistics learns beside its results (timed_run).
struct TimedRun {
    QueryKernelInfo kernel[2];      // the registers of the call's kernels, as `enqueue` reports them (most calls have one)
    unsigned long long counted[3];  // the counters behind the run
    uint32_t word;                  // the extra word behind the run
};

// The one run with statistics.  `enqueue(info)` puts the call's kernels on `stream` (info == nullptr) or reports the instantiations
// that would run into info[0 ..] instead.  The call gets `n_counters` 64-bit counters of its own (batches of one scene may run on
// several streams at once): `*slots[k]`, pointers among the kernels' arguments, are set to counter k before anything is enqueued --
// a kernel that takes an array of counters takes the last slot.  The counters are cleared, the kernels run between two events, the
// counters and `*word` (device memory, where not null: the advances' survivors) are copied to `run`, and the stream is waited for.
// The time and the first kernel's registers go to the members every family's statistics have.
template <class Enqueue, class Stats>
static int timed_run(Enqueue enqueue, std::initializer_list<unsigned long long **> slots, size_t n_counters, const uint32_t *word, int device,
                     hipStream_t stream, const char *who, Stats *stats, TimedRun &run)
{
    HIP_TRY(enqueue(run.kernel));
    DeviceArena scratch(device);
    unsigned long long *counters = nullptr;
    HIP_TRY(scratch.alloc(n_counters, counters));
    size_t k = 0;
    for (unsigned long long **slot : slots) *slot = counters + k++;
    // from here on the chain: the events are destroyed, and the stream waited for, whatever fails
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, n_counters * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
    if (e == hipSuccess) e = enqueue(nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(run.counted, counters, n_counters * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && word) e = hipMemcpyAsync(&run.word, word, sizeof run.word, hipMemcpyDeviceToHost, stream);
    const hipError_t waited = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = waited;
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (hipEvent_t v : ev)
        if (v) hipEventDestroy(v);
    if (e != hipSuccess) return hip_fail(e, who);
    stats->seconds = (double)ms * 1e-3;
    stats->kernel_vgprs = (uint32_t)run.kernel[0].vgprs;
    stats->scratch_bytes = (uint32_t)run.kernel[0].scratch_bytes;
    return RT_OK;
}

// Runs a lane-per-ray kernel on `stream` and waits for it: the kernel reads the scene's tables and the caller's arrays, and is
// done before either may change.  stats == nullptr: the launch and the wait alone; otherwise timed_run, whose arguments these are.
template <class Enqueue, class Stats>
static int run_lane_kernel(Enqueue enqueue, std::initializer_list<unsigned long long **> slots, size_t n_counters, int device, hipStream_t stream,
                           const char *who, Stats *stats, TimedRun &run)
{
    if (stats) return timed_run(enqueue, slots, n_counters, nullptr, device, stream, who, stats, run);
    hipError_t e = enqueue(nullptr);
    const hipError_t waited = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = waited;
    return e == hipSuccess ? RT_OK : hip_fail(e, who);
}

// The host arrays of one batch of `n` rays on the device (host_batch below); the copies are synchronous.
// `dev` comes in null: an input the caller left null, an output the caller does not want, stays so.
struct Staging {
    struct Out { void *host; const void *dev; size_t bytes_per_ray; };
    DeviceArena arena;
    size_t n;
    std::vector<Out> outs;
    hipError_t error = hipSuccess;  // the first failure of in() or out(), behind which neither does anything
    template <class T>
    void in(const T *host, size_t per_ray, const T *&dev)  // `per_ray` values a ray
    {
        if (host && error == hipSuccess) error = arena.upload(host, n * per_ray, dev);
    }
    template <class T>
    void out(T *host, size_t per_ray, T *&dev)  // room for them, remembered for fetch()
    {
        if (!host || error != hipSuccess) return;
        error = arena.alloc(n * per_ray, dev);
        if (error == hipSuccess) outs.push_back(Out{host, dev, per_ray * sizeof(T)});
    }
    hipError_t fetch(size_t rows) const  // the first `rows` rows of every remembered output back to its host array
    {
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < outs.size() && e == hipSuccess && rows; k++)
            e = hipMemcpy(outs[k].host, outs[k].dev, outs[k].bytes_per_ray * rows, hipMemcpyDeviceToHost);
        return e;
    }
};

// ---- the per-ray arrays of every rays struct and every outputs struct, stated once: member, values per ray, in or out ----
// Each walks a caller's struct of host arrays `h` and its zero-initialised twin `d`, which receives the device arrays.
static void stage_arrays(Staging &st, const rt_query_rays &h, rt_query_rays &d)
{
    st.in(h.origin, 3, d.origin);
    st.in(h.direction, 3, d.direction);
    st.in(h.time, 1, d.time);
    st.in(h.tmin, 1, d.tmin);
    st.in(h.tmax, 1, d.tmax);
}
static void stage_arrays(Staging &st, const rt_query_hits &h, rt_query_hits &d)
{
    st.out(h.t, 1, d.t);
    st.out(h.normal, 3, d.normal);
    st.out(h.uv, 2, d.uv);
    st.out(h.albedo, 3, d.albedo);
    st.out(h.leaf, 1, d.leaf);
    st.out(h.front_face, 1, d.front_face);
    st.out(h.material, 1, d.material);
    st.out(h.occluded, 1, d.occluded);
}
static void stage_arrays(Staging &st, const rt_radiance_rays &h, rt_radiance_rays &d)  // (radiance and radiance direct)
{
    st.in(h.origin, 3, d.origin);
    st.in(h.direction, 3, d.direction);
    st.in(h.time, 1, d.time);
    st.in(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_radiance_out &h, rt_radiance_out &d)
{
    st.out(h.radiance, 3, d.radiance);
    st.out(h.path_rays, 1, d.path_rays);
    st.out(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_path_step_rays &h, rt_path_step_rays &d)
{
    st.in(h.origin, 3, d.origin);
    st.in(h.direction, 3, d.direction);
    st.in(h.time, 1, d.time);
    st.in(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_path_step_out &h, rt_path_step_out &d)
{
    st.out(h.status, 1, d.status);
    st.out(h.emitted, 3, d.emitted);
    st.out(h.attenuation, 3, d.attenuation);
    st.out(h.origin, 3, d.origin);
    st.out(h.direction, 3, d.direction);
    st.out(h.time, 1, d.time);
    st.out(h.t, 1, d.t);
    st.out(h.normal, 3, d.normal);
    st.out(h.front_face, 1, d.front_face);
    st.out(h.material, 1, d.material);
    st.out(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_light_points &h, rt_light_points &d)
{
    st.in(h.point, 3, d.point);
    st.in(h.normal, 3, d.normal);
    st.in(h.material, 1, d.material);
    st.in(h.time, 1, d.time);
    st.in(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_light_samples &h, rt_light_samples &d)
{
    st.out(h.direction, 3, d.direction);
    st.out(h.distance, 1, d.distance);
    st.out(h.light, 1, d.light);
    st.out(h.pdf, 1, d.pdf);
    st.out(h.emitted, 3, d.emitted);
    st.out(h.scatter_pdf, 1, d.scatter_pdf);
    st.out(h.contribution, 3, d.contribution);
    st.out(h.rng_state, 6, d.rng_state);
}
static void stage_arrays(Staging &st, const rt_light_rays &h, rt_light_rays &d)
{
    st.in(h.origin, 3, d.origin);
    st.in(h.direction, 3, d.direction);
    st.in(h.time, 1, d.time);
}
static void stage_arrays(Staging &st, const rt_light_pdf_out &h, rt_light_pdf_out &d)
{
    st.out(h.pdf, 1, d.pdf);
    st.out(h.light, 1, d.light);
}
// the advances: the structs of the one with light samples begin with the plain one's fields (advance_args and advance_arrays_check
// below rely on the same), so these two serve both and the direct structs add their density.  The two count words and the
// `radiance` rows are no per-ray arrays: host_batch has them.
template <class Rays>
static void stage_advance_rays(Staging &st, const Rays &h, Rays &d)
{
    st.in(h.origin, 3, d.origin);
    st.in(h.direction, 3, d.direction);
    st.in(h.time, 1, d.time);
    st.in(h.rng_state, 6, d.rng_state);
    st.in(h.throughput, 3, d.throughput);
    st.in(h.ray_id, 1, d.ray_id);
    st.in(h.alive, 1, d.alive);
}
template <class Out>
static void stage_advance_out(Staging &st, const Out &h, Out &d)
{
    st.out(h.origin, 3, d.origin);
    st.out(h.direction, 3, d.direction);
    st.out(h.time, 1, d.time);
    st.out(h.rng_state, 6, d.rng_state);
    st.out(h.throughput, 3, d.throughput);
    st.out(h.ray_id, 1, d.ray_id);
    st.out(h.t, 1, d.t);
    st.out(h.normal, 3, d.normal);
    st.out(h.front_face, 1, d.front_face);
    st.out(h.material, 1, d.material);
}
static void stage_arrays(Staging &st, const rt_path_advance_rays &h, rt_path_advance_rays &d) { stage_advance_rays(st, h, d); }
static void stage_arrays(Staging &st, const rt_path_advance_out &h, rt_path_advance_out &d) { stage_advance_out(st, h, d); }
static void stage_arrays(Staging &st, const rt_path_advance_direct_rays &h, rt_path_advance_direct_rays &d)
{
    stage_advance_rays(st, h, d);
    st.in(h.scatter_pdf, 1, d.scatter_pdf);
}
static void stage_arrays(Staging &st, const rt_path_advance_direct_out &h, rt_path_advance_direct_out &d)
{
    stage_advance_out(st, h, d);
    st.out(h.scatter_pdf, 1, d.scatter_pdf);
}

template <class Params>
constexpr bool kIsAdvanceDirect = std::is_same<Params, rt_path_advance_direct_params>::value;
template <class Params>
constexpr bool kIsAdvance = std::is_same<Params, rt_path_advance_params>::value || kIsAdvanceDirect<Params>;

// The call on host arrays of every family, behind its check: the arrays are staged on the device, `device_call` -- the family's
// entry point on device arrays -- runs on them, and the outputs come back.
// The advances differ in what include/rtow.h states of their host form: the rows below the word rays->count alone travel, the
// `sources` rows of `radiance` go up and come back, the survivors' count and the workspace are this call's own, the call waits
// (the device call with statistics does), and the first *out->count rows of each output are copied back.
template <class Params, class Rays, class Out, class Stats>
static int host_batch(rt_scene *scene, const Params *p, const Rays *rays, const Out *out, Stats *stats,
                      int (*device_call)(rt_scene *, const Params *, const Rays *, const Out *, Stats *))
{
    if (stats) *stats = Stats{};
    if (p->count == 0) return RT_OK;
    if (int rc = select_device(p->device)) return rc;
    Params dp = *p;
    dp.stream = nullptr;  // the copies around the call are synchronous: nothing to order on the caller's stream
    if constexpr (kIsAdvance<Params>) {  // the host knows the word
        if (rays->count && (int64_t)*rays->count < p->count) dp.count = (int64_t)*rays->count;
        if (dp.count == 0) {
            *out->count = 0;
            return RT_OK;
        }
    }
    Staging stage{DeviceArena(p->device), (size_t)dp.count, {}};
    Rays dr{};
    Out dout{};
    stage_arrays(stage, *rays, dr);
    stage_arrays(stage, *out, dout);
    HIP_TRY(stage.error);
    if constexpr (kIsAdvance<Params>) {
        const size_t folded = out->radiance ? (size_t)p->sources * 3 : 0;
        if (folded) {
            const double *uploaded = nullptr;
            HIP_TRY(stage.arena.upload(out->radiance, folded, uploaded));
            dout.radiance = const_cast<double *>(uploaded);
        }
        HIP_TRY(stage.arena.alloc(1, dout.count));
        dp.workspace_bytes = kIsAdvanceDirect<Params> ? rt_path_advance_direct_workspace_bytes(dp.count) : rt_path_advance_workspace_bytes(dp.count);
        unsigned char *workspace = nullptr;
        HIP_TRY(stage.arena.alloc((size_t)dp.workspace_bytes, workspace));
        dp.workspace = workspace;
        Stats waited{};
        if (int rc = device_call(scene, &dp, &dr, &dout, stats ? stats : &waited)) return rc;
        uint32_t survivors = 0;
        HIP_TRY(hipMemcpy(&survivors, dout.count, sizeof survivors, hipMemcpyDeviceToHost));
        if (survivors > (uint32_t)dp.count) survivors = (uint32_t)dp.count;  // (never)
        HIP_TRY(stage.fetch(survivors));
        if (folded) HIP_TRY(hipMemcpy(out->radiance, dout.radiance, folded * sizeof(double), hipMemcpyDeviceToHost));
        *out->count = survivors;
    } else {
        if (int rc = device_call(scene, &dp, &dr, &dout, stats)) return rc;
        HIP_TRY(stage.fetch(stage.n));
    }
    return RT_OK;
}

extern "C" {

int rt_scene_upload(rt_scene *scene, int device)
{
    if (!scene) return fail(RT_ERR_INVALID, "rt_scene_upload: null scene");
    SceneImpl &s = *S(scene);
    if (!s.committed) return fail(RT_ERR_STATE, "rt_scene_upload: scene not committed (rt_scene_commit)");
    if (int rc = select_device(device)) return rc;
    if ((int)s.device.size() <= device) s.device.resize(device + 1, nullptr);
    if (s.device[device]) {
        if (s.device[device]->generation == s.generation) return RT_OK;
        // The scene was re-committed or its camera changed since this copy was made.  Nothing can still be reading
        // it: commit / set_camera refuse while a launch is in flight.
        release_device_tables(s.device[device]);
        s.device[device] = nullptr;
    }
    const FlatScene &f = s.flat;
    {
        // The packed scan's loop (render.hip scan_filtered32) takes its bounds from the segment records alone: they must tile the
        // table's trips exactly, in order, and none may be empty -- a loop that ran past its end would read beyond the table.
        const size_t trips = (f.sphere_scan.size() + 2 * kScanTripPairs - 1) / (2 * kScanTripPairs);
        size_t at = 0;
        bool tiled = f.sphere_scan32.size() == scan32_padded_pairs(f.sphere_scan.size());
        for (const ScanSegment &sg : f.scan_segments) {
            tiled = tiled && sg.first_trip == at && sg.n_trips > 0 && sg.axis <= kScanAxisNone;
            at += sg.n_trips;
        }
        if (!tiled || at != trips) return fail(RT_ERR_STATE, "rt_scene_upload: the scan segments do not tile the sphere table");
        // ... and its windows are read by segment and by trip index: a table is whole or absent
        if (!f.scan_windows.empty() && (f.scan_windows.size() != f.scan_segments.size() || f.scan_trip_spans.size() != trips))
            return fail(RT_ERR_STATE, "rt_scene_upload: the scan windows do not match the scan segments");
    }
    // The hit record reads quads[AAQuad::pad] for a marked triangle (render.hip vertex_attr): every mark must name an attribute row.
    for (const AAQuad &a : f.quad_aa)
        if (a.code == kQuadTriangle && a.pad && (a.pad < f.quads.size() || a.pad - f.quads.size() >= f.tri_attr.size()))
            return fail(RT_ERR_STATE, "rt_scene_upload: a triangle's attribute row lies outside the table");
    DeviceTables *dt = new DeviceTables;
    dt->memory = DeviceArena(device);
    dt->generation = s.generation;
    DeviceScene &d = dt->scene;
    hipError_t e = hipSuccess;
    auto up = [&](auto &host, auto &dev) {
        if (e == hipSuccess) e = dt->memory.upload(host, dev);
    };
    up(f.spheres, d.spheres);
    up(f.sphere_scan, d.sphere_scan);
    up(f.sphere_scan32, d.sphere_scan32);
    {
        // The scan segments and, directly behind them in the one allocation, the windows of the runs: a ScanWindowSeg per segment, then
        // a ScanTripSpan per trip (flat_scene.h).  The scan reaches the windows from the segments' pointer (render.hip scan_filtered32:
        // no register of its own across the loops), and only where a launch says that the scene has them.
        static_assert(sizeof(ScanWindowSeg) == sizeof(ScanSegment) && sizeof(ScanSegment) == 16 && sizeof(ScanTripSpan) == 8, "the windows are addressed in segment records");
        const size_t ns = f.scan_segments.size(), bytes = 2 * ns * sizeof(ScanSegment) + f.scan_trip_spans.size() * sizeof(ScanTripSpan);
        std::vector<unsigned char> table(bytes);
        if (ns) std::memcpy(table.data(), f.scan_segments.data(), ns * sizeof(ScanSegment));
        if (!f.scan_windows.empty()) {
            std::memcpy(table.data() + ns * sizeof(ScanSegment), f.scan_windows.data(), ns * sizeof(ScanWindowSeg));
            std::memcpy(table.data() + 2 * ns * sizeof(ScanSegment), f.scan_trip_spans.data(), f.scan_trip_spans.size() * sizeof(ScanTripSpan));
        } else {
            for (size_t k = 0; k < ns; k++) {
                const ScanWindowSeg none{kScanAxisNone, 0.0f, 0.0f, 0u};
                std::memcpy(table.data() + (ns + k) * sizeof(ScanSegment), &none, sizeof none);
            }
        }
        const unsigned char *dev = nullptr;
        up(table, dev);
        d.scan_segments = reinterpret_cast<const ScanSegment *>(dev);
        dt->scan_windows = !f.scan_windows.empty();
    }
    up(f.sphere_aux, d.sphere_aux);
    up(f.mspheres, d.mspheres);
    up(f.ms_planes, d.ms_planes);
    up(f.msphere_aux, d.msphere_aux);
    if (f.tri_attr.empty()) {
        up(f.quads, d.quads);
    } else {  // the attribute rows directly behind the quad rows, one allocation: quads[n_quads + k] is row k (flat_scene.h TriAttrRow)
        std::vector<QuadGeom> rows(f.quads.size() + f.tri_attr.size());
        std::memcpy(rows.data(), f.quads.data(), f.quads.size() * sizeof(QuadGeom));
        std::memcpy(rows.data() + f.quads.size(), f.tri_attr.data(), f.tri_attr.size() * sizeof(TriAttrRow));
        up(rows, d.quads);
    }
    up(f.quad_aa, d.quad_aa);
    up(f.boxes, d.boxes);
    up(f.quad_mat, d.quad_mat);
    up(f.objects, d.objects);
    up(f.items, d.items);
    up(f.xforms, d.xforms);
    up(f.media, d.media);
    up(f.group_boxes, d.group_boxes);
    up(f.tree_nodes, d.tree_nodes);
    up(f.tree_items, d.tree_items);
    up(f.tree_bvh, d.tree_bvh);
    up(f.nodes, d.nodes);
    up(f.fast_nodes, d.fast_nodes);
    up(f.fast_order, d.fast_order);
    {
        // The library tree's rows as the kernels read them: boxes in fp32, outwards (flat_scene.h FastNodeF).  The widening covers
        // what a conservative fp32 slab test can lose: the rounding of the box, of the ray's origin and of the products, each at
        // most 2^-23 of the magnitudes involved -- the scene's reach (every leaf box, the media's included: rays start on
        // surfaces, inside media or at the camera).
        double reach = 1.0;
        for (const Box &b : f.leaf_boxes)
            for (int a = 0; a < 3; a++) reach = std::fmax(reach, std::fmax(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
        for (int a = 0; a < 3; a++) reach = std::fmax(reach, std::fabs(s.camera.origin[a]) + std::fabs(s.camera.lens_radius) * 2.0);
        const double widen = reach * 1.9073486328125e-06;  // 2^-19
        auto down = [](double v) { float x = (float)v; return (double)x > v ? std::nextafterf(x, -INFINITY) : x; };
        auto up_f = [](double v) { float x = (float)v; return (double)x < v ? std::nextafterf(x, INFINITY) : x; };
        std::vector<FastNodeF> rows(f.fast_nodes.size());
        for (size_t k = 0; k < rows.size(); k++) {
            const FastNodeRec &n = f.fast_nodes[k];
            FastNodeF &r = rows[k];
            const double lo[3] = {n.xlo, n.ylo, n.zlo}, hi[3] = {n.xhi, n.yhi, n.zhi};
            for (int a = 0; a < 3; a++) {
                r.box[2 * a] = down(lo[a] - widen);
                r.box[2 * a + 1] = up_f(hi[a] + widen);
            }
            r.a = n.a;
            r.b = n.b;
            std::memcpy(r.link, n.link, sizeof r.link);
            r.pad = 0;
        }
        up(rows, d.fast_rows);
        std::vector<SegMedium> media = f.seg_media;
        for (SegMedium &m : media)
            for (int a = 0; a < 3; a++) {
                m.fbox[2 * a] = down(m.lo[a] - widen);
                m.fbox[2 * a + 1] = up_f(m.hi[a] + widen);
            }
        up(media, d.seg_media);
    }
    up(f.seg_cand, d.seg_cand);
    up(f.world_items, d.world_items);
    up(f.node_leaf_pos, dt->node_leaf_pos);
    up(f.lights, dt->lights);
    up(f.light_cdf[0], dt->light_cdf[0]);
    up(f.light_cdf[1], dt->light_cdf[1]);
    dt->n_lights = (uint32_t)f.lights.size();
    up(f.materials, d.materials);
    up(f.textures, d.textures);
    up(f.images, d.images);
    up(f.image_bytes, d.image_bytes);
    up(f.perlin, d.perlin);
    if (!(f.flags & SCENE_ENVIRONMENT)) {
        std::vector<CameraRec> cam_host(1, s.camera);
        up(cam_host, d.camera);
    } else {  // the environment's record directly behind the camera's, one allocation: camera + 1 (flat_scene.h EnvRec)
        static_assert(sizeof(CameraRec) % 8 == 0, "the record behind it holds doubles and pointers");
        EnvRec env = f.env;
        up(f.env_rgb, env.rgb);
        up(f.env_mcdf, env.mcdf);
        up(f.env_ccdf, env.ccdf);
        std::vector<unsigned char> both(sizeof(CameraRec) + sizeof(EnvRec));
        std::memcpy(both.data(), &s.camera, sizeof(CameraRec));
        std::memcpy(both.data() + sizeof(CameraRec), &env, sizeof(EnvRec));
        const unsigned char *dev = nullptr;
        up(both, dev);
        d.camera = reinterpret_cast<const CameraRec *>(dev);
    }
    if (e != hipSuccess) {
        release_device_tables(dt);
        return hip_fail(e, "rt_scene_upload: table upload");
    }
    scene_counts(f, d);
    d.scan_reach = f.scan_reach;
    d.scan_reach32 = f.scan_reach32;
    if (!(f.flags & SCENE_WORLD_MSPHERES)) d.ms_planes = nullptr;
    if (f.fast_nodes.empty()) d.fast_nodes = nullptr;
    s.device[device] = dt;
    return RT_OK;
}

rt_film *rt_film_create(int device, int width, int height, int stripe_rows, int rank, int world_size)
{
    if (width <= 0 || height <= 0 || stripe_rows <= 0 || world_size <= 0 || rank < 0 || rank >= world_size) {
        set_error("rt_film_create: bad geometry");
        return nullptr;
    }
    if ((int64_t)width * height >= (int64_t)1 << 31) {
        set_error("rt_film_create: frame too large (pixel index must fit in int like the reference's pixelIndex)");
        return nullptr;
    }
    if (select_device(device) != RT_OK) return nullptr;
    FilmImpl *f = new FilmImpl;
    f->device = device;
    f->planes = DeviceArena(device);
    f->stripe_rows = stripe_rows;
    f->rank = rank;
    f->world_size = world_size;
    f->geometry = film_geometry(width, height, stripe_rows, rank, world_size);
    const size_t np = f->plane_pixels();
    hipError_t e = f->planes.alloc(np * 3, f->own_pixels);
    if (e == hipSuccess) e = hipMemset(f->own_pixels, 0, np * 3 * sizeof(double));
    f->pixels = f->own_pixels;
    if (e == hipSuccess) e = f->planes.alloc(np * 6, f->state);
    if (e == hipSuccess) e = f->planes.alloc(kCounterWords, f->ray_counter);
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device);
        if (e == hipSuccess) f->num_cus = prop.multiProcessorCount;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = f->planes.alloc(f->geometry.n_tiles, f->tile_cost);
    if (e == hipSuccess) e = f->planes.alloc(f->geometry.n_tiles, f->tile_order);
    // (with the film, not on first use: an allocation between two launches' kernels would sit inside the frame's timed span)
    if (e == hipSuccess) e = f->planes.alloc((size_t)f->geometry.n_tiles * kPrimaryListWords, f->primary_lists);
    if (e == hipSuccess) e = hipHostMalloc((void **)&f->host_counters, kCounterWords * sizeof(unsigned long long), hipHostMallocDefault);
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventCreate(&f->ev[k]);
    if (e != hipSuccess) {
        hip_fail(e, "rt_film_create allocation");
        rt_film_destroy(reinterpret_cast<rt_film *>(f));
        return nullptr;
    }
    return reinterpret_cast<rt_film *>(f);
}

void rt_film_destroy(rt_film *film)
{
    if (!film) return;
    FilmImpl *f = F(film);
    hipSetDevice(f->device);
    if (f->in_flight) {  // destroyed without rt_render_finish: wait for the kernel, give the scene its count back
        if (f->last_stream) hipStreamSynchronize(f->last_stream);
        mark_done(*f);
    }
    if (f->host_counters) hipHostFree(f->host_counters);
    for (int k = 0; k < 4; k++)
        if (f->ev[k]) hipEventDestroy(f->ev[k]);
    if (f->own_stream) hipStreamDestroy(f->own_stream);
    delete f;  // and with it the planes
}

void *rt_film_device_pixels(rt_film *film) { return film ? F(film)->pixels : nullptr; }
size_t rt_film_pixel_bytes(rt_film *film) { return film ? (size_t)F(film)->geometry.n_pixels * 3 * sizeof(double) : 0; }
int rt_film_bind_pixels(rt_film *film, void *device_pixels)
{
    if (!film) return fail(RT_ERR_INVALID, "rt_film_bind_pixels: null film");
    if (F(film)->in_flight) return fail(RT_ERR_STATE, "rt_film_bind_pixels: a render is in flight");
    F(film)->pixels = device_pixels ? static_cast<double *>(device_pixels) : F(film)->own_pixels;
    return RT_OK;
}

// The strict and the fast build of render.hip, by rt_render_params::variant.
struct Build {
    hipError_t (*seed)(const SeedArgs &, hipStream_t);
    hipError_t (*render)(int, const DeviceScene &, const RenderArgs &, hipStream_t);
    hipError_t (*info)(int, const DeviceScene &, const RenderArgs &, KernelInfo *);
    hipError_t (*adaptive_rule)(const AdaptiveRule &, uint32_t, const uint32_t *, const double *, const double *, double *, uint8_t *, hipStream_t);
    hipError_t (*features)(const DeviceScene &, const FeatureArgs &, hipStream_t);
    hipError_t (*query)(const DeviceScene &, const QueryArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*radiance)(const DeviceScene &, const RadianceArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*step)(const DeviceScene &, const StepArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*advance)(const DeviceScene &, const AdvanceArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*light_sample)(const DeviceScene &, const LightArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*light_pdf)(const DeviceScene &, const LightArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*env_sample)(const DeviceScene &, const LightArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*env_pdf)(const DeviceScene &, const LightArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*advance_direct)(const DeviceScene &, const AdvanceDirectArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*advance_shadow)(const DeviceScene &, const AdvanceDirectArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*radiance_direct)(const DeviceScene &, const RadianceDirectArgs &, hipStream_t, QueryKernelInfo *);
    hipError_t (*film_direct)(const DeviceScene &, const FilmDirectArgs &, hipStream_t, FilmDirectInfo *);
};
static const Build kBuilds[2] = {
    {launch_seed_strict, launch_render_strict, kernel_info_strict, launch_adaptive_rule_strict, launch_features_strict, launch_query_strict,
     launch_radiance_strict, launch_step_strict, launch_advance_strict, launch_light_sample_strict, launch_light_pdf_strict,
     launch_env_sample_strict, launch_env_pdf_strict,
     launch_advance_direct_strict, launch_advance_shadow_strict, launch_radiance_direct_strict, launch_film_direct_strict},
    {launch_seed_fast, launch_render_fast, kernel_info_fast, launch_adaptive_rule_fast, launch_features_fast, launch_query_fast,
     launch_radiance_fast, launch_step_fast, launch_advance_fast, launch_light_sample_fast, launch_light_pdf_fast,
     launch_env_sample_fast, launch_env_pdf_fast,
     launch_advance_direct_fast, launch_advance_shadow_fast, launch_radiance_direct_fast, launch_film_direct_fast}};

static int seed_film(FilmImpl &f, const rt_render_params *p, hipStream_t stream)
{
    SeedArgs sa{};
    sa.state = f.state;
    if (int rc = device_jump_table(f.device, &sa.jump_table)) return rc;
    sa.base = xorwow_seed(p->seed, kSaltCurandDevice);
    sa.n_pixels = f.geometry.n_pixels;
    sa.width = f.geometry.width;
    sa.stripe_rows = f.stripe_rows;
    sa.rank = f.rank;
    sa.world_size = f.world_size;
    HIP_TRY(kBuilds[p->variant].seed(sa, stream));
    f.seeded = true;
    return RT_OK;
}

// Film bookkeeping: the frame this launch begins or adds to -- the running sums of an accumulated frame, the per-pixel
// planes of adaptive sampling -- and where the kernel finds them.
static int book_frame(FilmImpl &f, const rt_render_params *p, bool keep, bool continues, RenderArgs &ra, hipStream_t stream)
{
    if (p->flags & RT_FLAG_ACCUMULATE) {
        // progressive frame: this launch's samples are added to the film's running sums (needs the saved RNG streams)
        if (!f.accum) {
            HIP_TRY(f.planes.alloc(f.plane_pixels() * 3, f.accum));
            f.accum_spp = 0;
        }
        if (!keep) f.accum_spp = 0;  // re-seeded: start a new frame
        ra.accum = f.accum;
        ra.spp_before = f.accum_spp;
        if (p->samples_per_pixel > 0) f.accum_spp += p->samples_per_pixel;
        if (!continues) {  // what this frame is begun with, it has to be continued with (rt_render_launch)
            f.frame_adaptive = f.adaptive;
            f.frame_rule = f.rule;
        }
        f.frame_spp = f.accum_spp;
    } else {
        f.frame_spp = p->samples_per_pixel;
        // a launch without ACCUMULATE overwrites every pixel -- also the stopped ones of an accumulated adaptive frame, which no later
        // launch would write again: that frame has ended
        if (f.adaptive || f.frame_adaptive) f.accum_spp = 0;
    }
    if (f.adaptive) {
        // samples_per_pixel is the most a pixel may take in this launch; n, q and the mark live per pixel and persist with the
        // sums of an accumulated frame
        const size_t np = f.plane_pixels();
        if (!f.ad_n) {
            HIP_TRY(f.planes.alloc(np, f.ad_n));
            HIP_TRY(f.planes.alloc(np, f.ad_q));
            HIP_TRY(f.planes.alloc(np, f.ad_mark));
        }
        if (!continues) {
            HIP_TRY(hipMemsetAsync(f.ad_n, 0, np * sizeof(uint32_t), stream));
            HIP_TRY(hipMemsetAsync(f.ad_q, 0, np * sizeof(double), stream));
            HIP_TRY(hipMemsetAsync(f.ad_mark, 0, np, stream));
        }
        ra.adaptive = 1;
        ra.rule = f.rule;
        ra.ad_n = f.ad_n;
        ra.ad_q = f.ad_q;
        ra.ad_mark = f.ad_mark;
    }
    return RT_OK;
}

// The kernel's arguments from the film, the caller's params and the plan (launch_plan.h): no decision is taken here.
static void fill_render_args(const FilmImpl &f, const rt_render_params *p, const rt_launch_plan &plan, RenderArgs &ra)
{
    ra.pixels = f.pixels;
    ra.state = f.state;
    ra.ray_counter = f.ray_counter;
    ra.cursor = reinterpret_cast<uint32_t *>(f.ray_counter + 1);
    ra.coop_threshold = plan.coop_threshold;
    ra.coop_single = (p->flags & RT_FLAG_COOP_SINGLE) ? 1 : 0;
    ra.num_cus = f.num_cus;
    ra.shade_batch = plan.shade_batch;
    ra.max_blocks_per_cu = plan.max_blocks_per_cu;
    ra.pixels_per_wave = plan.pixels_per_wave;
    ra.boost_rounds = 8;
    ra.node_burst = plan.node_burst;
    ra.park_ratio = plan.park_ratio;
    ra.leaf_batch = plan.leaf_batch;
    ra.object_batch = plan.object_batch;
    ra.rounds = plan.rounds;
    ra.overdue_priority = (p->flags & RT_FLAG_OVERDUE_PRIORITY) ? 1 : 0;
    ra.ray_budget = plan.ray_budget;
    ra.n_pixels = f.geometry.n_pixels;
    ra.width = f.geometry.width;
    ra.height = f.geometry.height;
    ra.rows_owned = f.geometry.rows_owned;
    ra.spp = p->samples_per_pixel;
    ra.max_depth = p->max_depth;
    ra.stripe_rows = f.stripe_rows;
    ra.rank = f.rank;
    ra.world_size = f.world_size;
    ra.force_general = (p->flags & RT_FLAG_FORCE_GENERAL) ? 1 : 0;
    ra.always_walk = plan.always_walk;
    ra.reference_tree = plan.reference_tree;
    ra.exact_scan = (p->flags & RT_FLAG_EXACT_SCAN) ? 1 : 0;
    ra.accelerate_lists = plan.accelerate_lists;
    ra.filter_fp64 = (p->flags & RT_FLAG_FILTER_FP64) ? 1 : 0;
    ra.small_world = (int32_t)kSmallWorldScanCost;
}

// the planes the plan's pixel classes need (allocated on first use, kept with the film)
static int allocate_class_planes(FilmImpl &f, const rt_launch_plan &plan)
{
    if (!plan.pixel_classes) return RT_OK;
    if (!f.pix_cost) {
        HIP_TRY(f.planes.alloc(f.geometry.n_pixels, f.pix_cost));
        HIP_TRY(f.planes.alloc(f.geometry.n_pixels, f.heavy_list));
        HIP_TRY(f.planes.alloc(kHeavyCountWords, f.heavy_count));
        HIP_TRY(f.planes.alloc(f.geometry.n_pixels, f.pix_class));
    }
    if (plan.super_threshold > 0 && !f.super_list) HIP_TRY(f.planes.alloc(f.geometry.n_pixels, f.super_list));
    return RT_OK;
}

// The rehearsal and what follows from it (plan_frame has the reasons): the probe launch, the tiles ranked by its ray counts,
// the pixels classified by them; `ra` receives the order and the lists for the render launch.  Where the rehearsal keeps its
// samples (plan.probe_keeps) it is the frame's first probe_spp samples: it continues from and writes to the frame's running sums
// -- the film's, or a plane of the film's own for a frame that is not accumulated -- and `ra` becomes the launch of the rest.
static int enqueue_rehearsal(FilmImpl &f, const DeviceScene &ds, const rt_launch_plan &plan, const Build &build, RenderArgs &ra, hipStream_t stream)
{
    const bool keeps = plan.probe_keeps != 0;
    if (keeps && !ra.accum) {
        if (!f.carry) HIP_TRY(f.planes.alloc(f.plane_pixels() * 3, f.carry));
        ra.accum = f.carry;
        ra.spp_before = 0;
    }
    RenderArgs probe = ra;
    probe.probe = keeps ? 2 : 1;
    probe.adaptive = 0;  // the rehearsal is the plain kernel's
    probe.ad_n = nullptr;
    probe.ad_q = nullptr;
    probe.ad_mark = nullptr;
    probe.spp = plan.probe_spp;
    if (!keeps) {  // it only counts rays
        probe.accum = nullptr;
        probe.spp_before = 0;
    }
    probe.probe_ray_cap = plan.probe_ray_cap;
    probe.max_blocks_per_cu = plan.probe_max_blocks_per_cu;
    probe.tile_cost = plan.rank_tiles ? f.tile_cost : nullptr;
    probe.tile_order = nullptr;
    probe.pix_cost = plan.pixel_classes ? f.pix_cost : nullptr;
    if (plan.rank_tiles) HIP_TRY(hipMemsetAsync(f.tile_cost, 0, f.geometry.n_tiles * sizeof(uint32_t), stream));
    HIP_TRY(build.render(plan.probe_kernel, ds, probe, stream));
    if (plan.rank_tiles) {
        HIP_TRY(launch_tile_order(f.tile_cost, f.tile_order, f.geometry.n_tiles, (uint32_t)plan.tile_flatness_x8, stream));
        ra.tile_order = f.tile_order;
    }
    if (keeps) {
        // the rehearsed samples are the frame's, and so are their rays: only the (light) queue cursor starts again
        HIP_TRY(hipMemsetAsync(f.ray_counter + 1, 0, sizeof(unsigned long long), stream));
        ra.spp -= plan.probe_spp;
        ra.spp_before += plan.probe_spp;
        ra.resumed_spp = plan.probe_spp;
        if (plan.probe_ray_cap > 0) {  // the pixels the cap stopped saved nothing: the refill tells them by their cost
            ra.probe_ray_cap = plan.probe_ray_cap;
            ra.pix_cost = f.pix_cost;
        }
    } else {
        HIP_TRY(hipMemsetAsync(f.ray_counter, 0, 2 * sizeof(unsigned long long), stream));  // rays, (light) queue cursor
    }
    if (!plan.pixel_classes) return RT_OK;
    const bool longest = plan.super_threshold > 0;
    HIP_TRY(hipMemsetAsync(f.heavy_count, 0, kHeavyCountWords * sizeof(uint32_t), stream));
    HIP_TRY(launch_classify_pixels(f.pix_cost, f.geometry.n_pixels, (uint32_t)plan.heavy_threshold, f.pix_class, f.heavy_list, f.heavy_count, stream,
                                   longest ? f.super_list : nullptr, (uint32_t)plan.super_threshold, (uint32_t)f.geometry.width,
                                   (uint32_t)plan.near_percent, (uint32_t)plan.near_neighbours));
    if (longest) {
        HIP_TRY(hipMemsetAsync(f.ray_counter + 9, 0, sizeof(unsigned long long), stream));
        ra.super_list = f.super_list;
        ra.super_count = f.heavy_count + 1;
        ra.super_cursor = reinterpret_cast<uint32_t *>(f.ray_counter + 9);
        ra.super_ppw = plan.super_ppw;
    }
    HIP_TRY(hipMemsetAsync(f.ray_counter + 6, 0, sizeof(unsigned long long), stream));  // heavy queue cursor
    ra.heavy_list = f.heavy_list;
    ra.heavy_count = f.heavy_count;
    ra.heavy_cursor = reinterpret_cast<uint32_t *>(f.ray_counter + 6);
    ra.heavy_waves = plan.heavy_waves;
    ra.heavy_ppw = plan.heavy_ppw;
    ra.heavy_priority = plan.heavy_priority;
    ra.adaptive_ppw = plan.adaptive_ppw;
    ra.pix_class = f.pix_class;
    return RT_OK;
}

// What every launch of a frame, plain or with light samples, puts on the stream first: the counters zeroed, the seeding between
// its two events, the film's bookkeeping (book_frame fills its part of `ra`) ...
static int enqueue_frame_begin(FilmImpl &f, const rt_render_params *p, RenderArgs &ra, hipStream_t stream)
{
    const bool keep = (p->flags & RT_FLAG_KEEP_RNG_STATE) && f.seeded;
    const bool continues = continues_frame(f, p);
    HIP_TRY(hipMemsetAsync(f.ray_counter, 0, kCounterWords * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(f.ev[0], stream));
    if (!keep)
        if (int rc = seed_film(f, p, stream)) return rc;
    HIP_TRY(hipEventRecord(f.ev[1], stream));
    return book_frame(f, p, keep, continues, ra, stream);
}
// ... and last, behind its kernels: the event, the counter copy, the event rt_render_finish waits for.
static int enqueue_frame_end(FilmImpl &f, hipStream_t stream)
{
    HIP_TRY(hipEventRecord(f.ev[2], stream));
    // The counters come home on the film's own stream: a blocking hipMemcpy in rt_render_finish would wait for every
    // other film's frame as well and serialise frames that were launched to overlap.
    HIP_TRY(hipMemcpyAsync(f.host_counters, f.ray_counter, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(f.ev[3], stream));
    return RT_OK;
}

// Everything rt_render_launch puts on the stream: seeding, the rehearsal and its bookkeeping, the render kernel, the
// counter copy.  Called with the film already marked in flight (a failure half-way leaves kernels running).  What runs and
// how is plan_launch's decision (launch_plan.h); this function carries it out.
static int enqueue_frame(SceneImpl &s, FilmImpl &f, const rt_render_params *p, hipStream_t stream)
{
    const Build &build = kBuilds[p->variant];
    const DeviceScene &ds = s.device[f.device]->scene;

    RenderArgs ra{};
    if (int rc = enqueue_frame_begin(f, p, ra, stream)) return rc;
    const rt_launch_plan plan = plan_launch(ds, f.geometry, f.num_cus, *p, f.adaptive, hits_stay_in_boxes(s.flat, s.camera, p->variant));
    fill_render_args(f, p, plan, ra);
    ra.scan_windows = !(p->flags & RT_FLAG_NO_SCAN_WINDOWS) && s.device[f.device]->scan_windows ? 1 : 0;  // sphere lists: the windows of the scan's runs
    KernelInfo info{};
    HIP_TRY(build.info(plan.kernel, ds, ra, &info));  // the registers the compiler gave it; the rest is the plan's
    if (info.kind != plan.kernel_kind || info.lds_bytes != plan.lds_bytes)
        return fail(RT_ERR_STATE, "rt_render_launch: the kernel is not the one the launch plan describes");
    f.last_plan = plan;
    f.last_kernel = info;
    if (int rc = allocate_class_planes(f, plan)) return rc;
    // Sphere lists: the candidates of every tile's camera rays, for the rehearsal and the frame launch alike.  Built by every
    // launch that can read them -- one lane per ray, and a full wave reaches the pixel-parallel scan (render_kernel's own condition
    // for a primary round): the camera and the scene may have changed since the last one, and the film has no key that would tell.
    if (is_sphere_list_kernel(plan.kernel_kind) && p->max_depth > 0 && !(p->flags & (RT_FLAG_EXACT_SCAN | RT_FLAG_NO_PRIMARY_LISTS)) &&
        plan.pixels_per_wave >= 64 && plan.coop_threshold <= 64 && ds.n_spheres <= 0xFFFFu && f.geometry.n_tiles > 0) {
        HIP_TRY(launch_primary_lists(ds, f.primary_lists, f.geometry.n_tiles, f.geometry.width, f.geometry.height, f.geometry.rows_owned,
                                     f.stripe_rows, f.rank, f.world_size, stream));
        ra.primary_lists = f.primary_lists;
    }
    if (plan.probe_spp > 0)
        if (int rc = enqueue_rehearsal(f, ds, plan, build, ra, stream)) return rc;
    HIP_TRY(build.render(plan.kernel, ds, ra, stream));
    return enqueue_frame_end(f, stream);
}

// Everything rt_render_launch_direct puts on the stream: what every frame launch begins and ends with, and between them the one
// kernel -- no rehearsal, no pixel classes, no primary lists.  The light table is the copy rt_scene_radiance_direct_device reads.
static int enqueue_frame_direct(SceneImpl &s, FilmImpl &f, const rt_render_params *p, const rt_film_direct_params *direct, hipStream_t stream)
{
    const Build &build = kBuilds[p->variant];
    const DeviceTables &dt = *s.device[f.device];

    RenderArgs ra{};
    if (int rc = enqueue_frame_begin(f, p, ra, stream)) return rc;
    FilmDirectArgs da{};
    da.pixels = f.pixels;
    da.accum = ra.accum;
    da.spp_before = ra.spp_before;
    da.state = f.state;
    da.ray_counter = f.ray_counter;
    da.cursor = reinterpret_cast<uint32_t *>(f.ray_counter + 1);
    da.n_pixels = f.geometry.n_pixels;
    da.width = f.geometry.width;
    da.height = f.geometry.height;
    da.rows_owned = f.geometry.rows_owned;
    da.spp = p->samples_per_pixel;
    da.max_depth = p->max_depth;
    da.stripe_rows = f.stripe_rows;
    da.rank = f.rank;
    da.world_size = f.world_size;
    da.num_cus = f.num_cus;
    da.max_blocks_per_cu = p->max_blocks_per_cu;
    da.adaptive = ra.adaptive;
    da.rule = ra.rule;
    da.ad_n = ra.ad_n;
    da.ad_q = ra.ad_q;
    da.ad_mark = ra.ad_mark;
    da.rows = dt.lights;
    da.cdf = dt.light_cdf[direct->strategy];
    da.n_lights = dt.n_lights;
    da.node_leaf_pos = dt.node_leaf_pos;
    da.shadow_counters = f.ray_counter + kShadowCounterWord;
    FilmDirectInfo info{};
    HIP_TRY(build.film_direct(dt.scene, da, stream, &info));
    f.last_plan = rt_launch_plan{};
    f.last_plan.pixels_per_wave = 64;
    f.last_plan.kernel_kind = info.kernel.kind;
    f.last_plan.lds_bytes = info.kernel.lds_bytes;
    f.last_kernel = info.kernel;
    f.last_direct_scratch = info.scratch_bytes;
    HIP_TRY(build.film_direct(dt.scene, da, stream, nullptr));
    return enqueue_frame_end(f, stream);
}

// everything a frame launch refuses without a device, in the order include/rtow.h lists it
static int frame_launch_check(rt_scene *scene, rt_film *film, const rt_render_params *p, const std::string &who)
{
    if (!scene || !film || !p) return fail(RT_ERR_INVALID, who + ": null argument");
    FilmImpl &f = *F(film);
    if (p->width != f.geometry.width || p->height != f.geometry.height || p->stripe_rows != f.stripe_rows || p->rank != f.rank ||
        p->world_size != f.world_size || p->device != f.device)
        return fail(RT_ERR_INVALID, who + ": params do not match the film's geometry/device");
    if (p->samples_per_pixel < 0 || p->max_depth < 0) return fail(RT_ERR_INVALID, who + ": negative spp/depth");
    if (p->variant != 0 && p->variant != 1) return fail(RT_ERR_INVALID, who + ": variant must be 0 (strict) or 1 (fast)");
    if (p->pixels_per_wave < 0 || p->pixels_per_wave > 64) return fail(RT_ERR_INVALID, who + ": pixels_per_wave must be 0 (automatic) or 1..64");
    if (f.in_flight)
        return fail(RT_ERR_STATE, who + ": this film already has a render in flight (rt_render_finish it first; "
                                        "use one film per frame in flight)");
    if (continues_frame(f, p) && (f.adaptive != f.frame_adaptive || (f.adaptive && !same_rule(f.rule, f.frame_rule))))
        return fail(RT_ERR_STATE, who + ": adaptive sampling was switched or given other parameters in the middle of an "
                                        "accumulated frame (begin a frame by re-seeding, or set it back)");
    return RT_OK;
}

// rt_render_launch and rt_render_launch_direct behind their checks (direct == nullptr: the plain launch)
static int launch_frame(rt_scene *scene, rt_film *film, const rt_render_params *p, const rt_film_direct_params *direct)
{
    SceneImpl &s = *S(scene);
    FilmImpl &f = *F(film);
    if (int rc = rt_scene_upload(scene, f.device)) return rc;
    if (int rc = select_device(f.device)) return rc;
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : f.own_stream;
    // In flight from here on: the scene may not change (or go away) under a kernel that is already on the stream, also
    // when a later step of the launch fails.
    f.last_stream = stream;
    mark_in_flight(s, f);
    const int rc = direct ? enqueue_frame_direct(s, f, p, direct, stream) : enqueue_frame(s, f, p, stream);
    if (rc != RT_OK) {
        const std::string why = rt_last_error();
        hipStreamSynchronize(stream);  // whatever did get enqueued
        mark_done(f);
        f.seeded = false;  // a rehearsal that ran has advanced the streams by part of a frame: the next launch seeds again
        set_error(why);
        return rc;
    }
    f.last_samples = (uint64_t)f.geometry.n_pixels * (uint64_t)p->samples_per_pixel;
    f.last_variant = p->variant;
    f.last_adaptive = f.adaptive;
    f.last_direct = direct != nullptr;
    f.rendered = true;
    return RT_OK;
}

int rt_render_launch(rt_scene *scene, rt_film *film, const rt_render_params *p)
{
    if (int rc = frame_launch_check(scene, film, p, "rt_render_launch")) return rc;
    return launch_frame(scene, film, p, nullptr);
}

int rt_render_launch_direct(rt_scene *scene, rt_film *film, const rt_render_params *p, const rt_film_direct_params *direct)
{
    const std::string who = "rt_render_launch_direct";
    if (int rc = frame_launch_check(scene, film, p, who)) return rc;
    if (!direct) return fail(RT_ERR_INVALID, who + ": direct is NULL");
    if (direct->strategy != 0 && direct->strategy != 1) return fail(RT_ERR_INVALID, who + ": strategy must be 0 (uniform) or 1 (by area and brightness)");
    for (int32_t word : direct->reserved)
        if (word != 0) return fail(RT_ERR_INVALID, who + ": reserved must be 0");
    return launch_frame(scene, film, p, direct);
}

int rt_film_last_direct_stats(rt_film *film, rt_film_direct_stats *out)
{
    if (!film || !out) return fail(RT_ERR_INVALID, "rt_film_last_direct_stats: null argument");
    const FilmImpl &f = *F(film);
    if (!f.has_direct_stats) return fail(RT_ERR_STATE, "rt_film_last_direct_stats: no direct launch of this film has been finished");
    *out = f.direct_stats;
    return RT_OK;
}

void rt_film_direct_abi_sizes(uint32_t out2[2])
{
    out2[0] = (uint32_t)sizeof(rt_film_direct_params);
    out2[1] = (uint32_t)sizeof(rt_film_direct_stats);
}

#if RT_PHASES  // diagnostic builds (make EXTRA=-DRT_PHASES=1 LIBNAME=...): the per-phase table
static void print_phases(const FilmImpl &f)
{
    const unsigned long long *c = f.host_counters;
    const char *name[24] = {"node step", "leaf test", "shade", "refill", "  group/instance", "  medium", "  primitive", "",
                            "    record+xforms", "    box", "    sub-BVH", "    other geometry", "between walks again", "limited node pass", "node visits (lanes)", "",
                            "box pass", "medium pass / between walks", "object pass", "primitive pass", "  hit record", "  scatter",
                            "  next camera ray", "  pixel done"};
    if (is_sphere_list_kernel(f.last_kernel.kind)) {  // slots 0 / 1 are its two scans
        name[0] = "scan, pixel-parallel";
        name[1] = "scan, cooperative";
        name[12] = name[13] = "";  // slots 12, 13, 15: the survivor counts of the pixel-parallel scan (render.hip ScanSums)
        const double passes = (double)c[96 + 0], groups = (double)c[96 + 12], taken = (double)c[64 + 12];
        if (groups > 0) {
            std::fprintf(stderr, "survivors: %.0f passes, %.2f groups of 4 per pass, groups taken f = %.4f\n", passes, groups / passes, taken / groups);
            std::fprintf(stderr, "survivors: spheres with a passing lane per taken group %.3f, lane appends per pass %.1f, lanes behind per pass %.2f\n",
                         (double)c[32 + 12] / taken, (double)c[96 + 13] / passes, (double)c[64 + 13] / passes);
            std::fprintf(stderr, "survivors: drains per pass %.2f, drain iterations (wave max of count) per pass %.2f, drain cycles %.1f %% of the "
                         "pixel-parallel scan's (%.0f of %.0f per pass)\n", (double)c[96 + 15] / passes, (double)c[64 + 15] / passes,
                         100.0 * c[32 + 13] / c[32 + 0], (double)c[32 + 13] / passes, (double)c[32 + 0] / passes);
        }
        name[19] = "";  // slot 19: camera rays among the live lanes of a pixel-parallel pass
        if (c[96 + 19])
            std::fprintf(stderr, "camera rays: %llu pixel-parallel passes, %.2f live lanes per pass, %.2f of them with a camera ray (depth 0): share %.4f\n",
                         c[96 + 19], (double)c[64 + 19] / c[96 + 19], (double)c[32 + 19] / c[96 + 19], (double)c[32 + 19] / (double)c[64 + 19]);
        name[23] = "";  // slot 23 and the cycle word of slot 15: the primary rounds (render.hip render_kernel)
        if (c[96 + 23])
            std::fprintf(stderr, "primary: %llu rounds, %.2f fresh lanes per round, %.2f list entries tested per round (%.2f per lane), %.0f cycles per round "
                         "(%.1f %% of wave time)\n", c[96 + 23], (double)c[64 + 23] / c[96 + 23], (double)c[32 + 15] / c[96 + 23],
                         (double)c[32 + 15] / (double)c[64 + 23], (double)c[32 + 23] / c[96 + 23], 100.0 * c[32 + 23] / (double)c[7]);
        // slots 14 and 7: the windows of the pixel-parallel scan's runs (render.hip ScanSums win_*).  Both are per-lane slots, which the
        // flush sums over the wave and scales by 1 / 1024: the counts come back times 64 / 1024, the ratios as they are.
        name[14] = name[7] = "";
        if (c[96 + 7])
            std::fprintf(stderr, "window: %llu windowed passes (%llu windowed runs), %.2f trips scanned per pass in them, %.2f ranges per pass, %.0f cycles "
                         "of window computation per pass\n", c[96 + 7] * 16ull, c[96 + 14] * 16ull, (double)c[64 + 14] / c[96 + 7], (double)c[64 + 7] / c[96 + 7],
                         (double)c[32 + 14] / c[96 + 7]);
        if (c[96 + 7])  // the cycle word of slot 7: what the lanes' OWN extents need of those runs (a work-item form's trips)
            std::fprintf(stderr, "window: %.1f lane-trips per windowed pass by each lane's own extent (sum over the live lanes), %.2f a live lane\n",
                         (double)c[32 + 7] / c[96 + 7], c[64 + 19] ? (double)c[32 + 7] / c[96 + 7] / ((double)c[64 + 19] / c[96 + 19]) : 0.0);
        name[16] = name[17] = name[18] = "";  // slots 16, 17, 18: the counts of the grouped scan (render.hip GroupedSums)
        const double gp = (double)c[96 + 16];
        if (gp > 0) {
            std::fprintf(stderr, "grouped: %.0f passes through the filter, %.2f rays per pass, exact-test blocks executed per pass %.2f\n", gp,
                         (double)c[64 + 16] / gp, (double)c[32 + 16] / gp);
            std::fprintf(stderr, "grouped: survivors (lanes tested) per pass %.2f, largest per-lane count per pass %.2f, drains per pass %.2f\n",
                         (double)c[32 + 17] / gp, (double)c[64 + 17] / gp, (double)c[96 + 17] / gp);
            std::fprintf(stderr, "grouped: cycles per pass: filter %.0f, exact tests %.0f (%.1f %% and %.1f %% of the cooperative scans' %.0f)\n",
                         (double)c[64 + 18] / gp, (double)c[32 + 18] / gp, 100.0 * c[64 + 18] / c[32 + 1], 100.0 * c[32 + 18] / c[32 + 1],
                         (double)c[32 + 1] / (double)c[96 + 1]);
            // the packed fp32 branch queues its survivors: there "blocks" above are drain iterations and "survivors" appends
            std::fprintf(stderr, "grouped: appends per pass %.2f, drains per pass %.2f, drain iterations per pass %.2f\n", (double)c[32 + 17] / gp,
                         (double)c[96 + 17] / gp, (double)c[32 + 16] / gp);
        }
    }
    const double total = (double)c[7];
    for (int k = 0; k < 24; k++)
        if (name[k][0] && c[96 + k])
            std::fprintf(stderr, "phase %-20s: %5.1f %% of wave time, %10llu passes, %5.1f lanes/pass, %7.0f cycles/pass\n", name[k],
                         100.0 * c[32 + k] / total, c[96 + k], (double)c[64 + k] / c[96 + k], (double)c[32 + k] / c[96 + k]);
}
#endif

int rt_render_finish(rt_scene *scene, rt_film *film, rt_render_stats *stats)
{
    (void)scene;
    if (!film) return fail(RT_ERR_INVALID, "rt_render_finish: null film");
    FilmImpl &f = *F(film);
    if (!f.in_flight) return fail(RT_ERR_STATE, "rt_render_finish: nothing launched");
    if (int rc = select_device(f.device)) return rc;
    const hipError_t waited = hipEventSynchronize(f.ev[3]);
    if (waited != hipSuccess && f.last_stream) hipStreamSynchronize(f.last_stream);  // whatever is left on the stream
    mark_done(f);  // also when the wait failed: the scene must not stay locked for ever
    if (waited != hipSuccess) return hip_fail(waited, "hipEventSynchronize(render finished)");
    if (f.last_direct) {
        f.direct_stats = rt_film_direct_stats{f.host_counters[kShadowCounterWord], f.host_counters[kShadowCounterWord + 1], (uint32_t)f.last_direct_scratch, 0u};
        f.has_direct_stats = true;
    }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        float ms_seed = 0, ms_render = 0;
        HIP_TRY(hipEventElapsedTime(&ms_seed, f.ev[0], f.ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_render, f.ev[1], f.ev[2]));
        const unsigned long long rays = f.host_counters[0];
#if RT_PHASES
        print_phases(f);
#endif
        stats->samples = f.last_adaptive ? (uint64_t)f.host_counters[2] : f.last_samples;  // adaptive: what the waves counted
        stats->rays = rays;
        stats->seconds_seed = ms_seed * 1e-3;
        stats->seconds_render = ms_render * 1e-3;
        stats->pixels = f.geometry.n_pixels;
        stats->rows = (uint32_t)f.geometry.rows_owned;
        stats->kernel_vgprs = (uint32_t)f.last_kernel.vgprs;
        stats->lds_bytes = (uint32_t)f.last_kernel.lds_bytes;
        stats->kernel_kind = (uint32_t)f.last_kernel.kind;
        stats->pixels_per_wave = (uint32_t)f.last_plan.pixels_per_wave;
    }
    return RT_OK;
}

int rt_film_download(rt_film *film, double *frame_full, int width, int height)
{
    if (!film || !frame_full) return fail(RT_ERR_INVALID, "rt_film_download: null argument");
    FilmImpl &f = *F(film);
    if (width != f.geometry.width || height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_download: frame size mismatch");
    if (int rc = select_device(f.device)) return rc;
    return download_rows(f, f.pixels, 3, false, frame_full);
}

int rt_film_set_adaptive(rt_film *film, const rt_adaptive_params *params)
{
    if (!film) return fail(RT_ERR_INVALID, "rt_film_set_adaptive: null film");
    FilmImpl &f = *F(film);
    if (f.in_flight) return fail(RT_ERR_STATE, "rt_film_set_adaptive: a render is in flight");
    if (params && !rule_in_range(*params))
        return fail(RT_ERR_INVALID, "rt_film_set_adaptive: needs min_samples >= 2, check_interval >= 1, noise_threshold >= 0, luminance_floor > 0");
    f.adaptive = params != nullptr;
    if (params) f.rule = to_rule(*params);
    return RT_OK;
}

int rt_film_download_sample_counts(rt_film *film, uint32_t *counts_full, int width, int height)
{
    if (!film || !counts_full) return fail(RT_ERR_INVALID, "rt_film_download_sample_counts: null argument");
    FilmImpl &f = *F(film);
    if (width != f.geometry.width || height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_download_sample_counts: frame size mismatch");
    if (f.in_flight) return fail(RT_ERR_STATE, "rt_film_download_sample_counts: a render is in flight");
    if (int rc = select_device(f.device)) return rc;
    if (f.rendered && f.last_adaptive) return download_rows(f, f.ad_n, 1, true, counts_full);
    // without adaptive sampling every owned pixel has had the frame's samples: nothing to fetch
    const std::vector<uint32_t> compact((size_t)f.geometry.n_pixels, f.rendered ? (uint32_t)f.frame_spp : 0u);
    scatter_owned_rows(compact.data(), 1, width, height, f.stripe_rows, f.rank, f.world_size, true, counts_full);
    return RT_OK;
}

int rt_film_download_probe_costs(rt_film *film, uint32_t *costs_full, int width, int height)
{
    if (!film || !costs_full) return fail(RT_ERR_INVALID, "rt_film_download_probe_costs: null argument");
    FilmImpl &f = *F(film);
    if (width != f.geometry.width || height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_download_probe_costs: frame size mismatch");
    if (f.in_flight) return fail(RT_ERR_STATE, "rt_film_download_probe_costs: a render is in flight");
    if (!f.rendered || !f.last_plan.pixel_classes || !f.pix_cost)
        return fail(RT_ERR_STATE, "rt_film_download_probe_costs: the film's last launch classified no pixels");
    if (int rc = select_device(f.device)) return rc;
    return download_rows(f, f.pix_cost, 1, true, costs_full);
}

int rt_adaptive_converged(const rt_adaptive_params *p, uint32_t n, double sum_r, double sum_g, double sum_b, double sum_y2)
{
    if (!p || !rule_in_range(*p)) {
        set_error("rt_adaptive_converged: needs min_samples >= 2, check_interval >= 1, noise_threshold >= 0, luminance_floor > 0");
        return -(int)RT_ERR_INVALID;
    }
    return adaptive_converged(to_rule(*p), n, sum_r, sum_g, sum_b, sum_y2) ? 1 : 0;
}

int rt_adaptive_rule_on_device(int device, int variant, const rt_adaptive_params *p, uint32_t count, const uint32_t *n,
                               const double *sums_rgbq, const double *sample_rgb, double *q_out, uint8_t *stops_out)
{
    if (!p || !rule_in_range(*p) || (variant != 0 && variant != 1) || (count && (!n || !sums_rgbq || !sample_rgb || !q_out || !stops_out)))
        return fail(RT_ERR_INVALID, "rt_adaptive_rule_on_device: bad argument");
    if (count == 0) return RT_OK;
    if (int rc = select_device(device)) return rc;
    DeviceArena scratch(device);
    const uint32_t *d_n = nullptr;
    const double *d_sums = nullptr, *d_sample = nullptr;
    double *d_q = nullptr;
    uint8_t *d_stops = nullptr;
    HIP_TRY(scratch.upload(n, count, d_n));
    HIP_TRY(scratch.upload(sums_rgbq, (size_t)count * 4, d_sums));
    HIP_TRY(scratch.upload(sample_rgb, (size_t)count * 3, d_sample));
    HIP_TRY(scratch.alloc(count, d_q));
    HIP_TRY(scratch.alloc(count, d_stops));
    HIP_TRY(kBuilds[variant].adaptive_rule(to_rule(*p), count, d_n, d_sums, d_sample, d_q, d_stops, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(q_out, d_q, count * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(stops_out, d_stops, count, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- first-hit feature buffers and the a-trous filter ----
static const char *denoise_params_error(const rt_denoise_params *p)
{
    if (!p) return "null params";
    if (p->iterations < 1 || p->iterations > 8) return "iterations must be 1..8";
    for (double sigma : {p->sigma_color, p->sigma_albedo, p->sigma_normal, p->sigma_depth})
        if (!(sigma > 0.0)) return "every sigma must be > 0 (+inf switches its term off)";  // (a NaN fails the comparison)
    return nullptr;
}

// The levels of the filter over full-frame device planes: level 0 reads `color`, the last level writes `out`, the ones between
// alternate between `out` and `tmp` (tmp may be null for a single level).  color, out and tmp are distinct.
static int enqueue_atrous(const double *color, const double *albedo, const double *normal, const double *depth, int width, int height,
                          const rt_denoise_params &p, double *out, double *tmp, hipStream_t stream)
{
    auto inv_sq = [](double sigma) { return 1.0 / (sigma * sigma); };  // +inf: 0
    AtrousArgs a{};
    a.albedo = albedo;
    a.normal = normal;
    a.depth = depth;
    a.width = width;
    a.height = height;
    a.inv_albedo = inv_sq(p.sigma_albedo);
    a.inv_normal = inv_sq(p.sigma_normal);
    a.inv_depth = inv_sq(p.sigma_depth);
    const double *in = color;
    for (int k = 0; k < p.iterations; k++) {
        double *dst = ((p.iterations - 1 - k) % 2 == 0) ? out : tmp;  // the last level lands in `out`
        a.in = in;
        a.out = dst;
        a.step = 1 << k;
        a.inv_color = inv_sq(p.sigma_color * std::ldexp(1.0, -k));
        HIP_TRY(launch_atrous(a, stream));
        in = dst;
    }
    return RT_OK;
}

int rt_film_render_features(rt_scene *scene, rt_film *film, const rt_feature_params *p)
{
    if (!scene || !film || !p) return fail(RT_ERR_INVALID, "rt_film_render_features: null argument");
    SceneImpl &s = *S(scene);
    FilmImpl &f = *F(film);
    if (p->width != f.geometry.width || p->height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_render_features: params do not match the film's size");
    if (p->samples < 0) return fail(RT_ERR_INVALID, "rt_film_render_features: negative samples");
    if (p->variant != 0 && p->variant != 1) return fail(RT_ERR_INVALID, "rt_film_render_features: variant must be 0 (strict) or 1 (fast)");
    if (f.in_flight) return fail(RT_ERR_STATE, "rt_film_render_features: a render of this film is in flight (rt_render_finish it first)");
    if (int rc = rt_scene_upload(scene, f.device)) return rc;
    if (int rc = select_device(f.device)) return rc;
    const size_t np = f.plane_pixels();
    if (!f.feat_albedo) HIP_TRY(f.planes.alloc(np * 3, f.feat_albedo));
    if (!f.feat_normal) HIP_TRY(f.planes.alloc(np * 3, f.feat_normal));
    if (!f.feat_depth) HIP_TRY(f.planes.alloc(np, f.feat_depth));
    FeatureArgs fa{};
    fa.albedo = f.feat_albedo;
    fa.normal = f.feat_normal;
    fa.depth = f.feat_depth;
    if (int rc = device_jump_table(f.device, &fa.jump_table)) return rc;
    fa.base = xorwow_seed(p->seed, kSaltCurandDevice);
    fa.n_pixels = f.geometry.n_pixels;
    fa.width = f.geometry.width;
    fa.height = f.geometry.height;
    fa.samples = p->samples;
    fa.stripe_rows = f.stripe_rows;
    fa.rank = f.rank;
    fa.world_size = f.world_size;
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : f.own_stream;
    const DeviceScene &ds = s.device[f.device]->scene;
    HIP_TRY(kBuilds[p->variant].features(ds, fa, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the kernel reads the scene's tables: done before the caller may change them
    f.has_features = true;
    f.has_denoised = false;
    return RT_OK;
}

int rt_film_download_features(rt_film *film, double *albedo_full, double *normal_full, double *depth_full, int width, int height)
{
    if (!film) return fail(RT_ERR_INVALID, "rt_film_download_features: null film");
    FilmImpl &f = *F(film);
    if (width != f.geometry.width || height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_download_features: frame size mismatch");
    if (!f.has_features) return fail(RT_ERR_STATE, "rt_film_download_features: no feature pass has run on this film (rt_film_render_features)");
    if (int rc = select_device(f.device)) return rc;
    if (albedo_full)
        if (int rc = download_rows(f, f.feat_albedo, 3, true, albedo_full)) return rc;
    if (normal_full)
        if (int rc = download_rows(f, f.feat_normal, 3, true, normal_full)) return rc;
    if (depth_full)
        if (int rc = download_rows(f, f.feat_depth, 1, true, depth_full)) return rc;
    return RT_OK;
}

void *rt_film_device_features(rt_film *film, int which)
{
    if (!film || !F(film)->has_features) return nullptr;
    return which == 0 ? F(film)->feat_albedo : which == 1 ? F(film)->feat_normal : which == 2 ? F(film)->feat_depth : nullptr;
}

int rt_film_denoise(rt_film *film, const rt_denoise_params *p)
{
    if (!film) return fail(RT_ERR_INVALID, "rt_film_denoise: null film");
    if (const char *why = denoise_params_error(p)) return fail(RT_ERR_INVALID, std::string("rt_film_denoise: ") + why);
    FilmImpl &f = *F(film);
    if (f.world_size > 1)
        return fail(RT_ERR_UNSUPPORTED, "rt_film_denoise: this film owns only part of the frame, its pixels' neighbours live on other "
                                        "ranks (gather the planes and use rt_denoise_frame)");
    if (f.in_flight) return fail(RT_ERR_STATE, "rt_film_denoise: a render of this film is in flight (rt_render_finish it first)");
    if (!f.has_features) return fail(RT_ERR_STATE, "rt_film_denoise: no feature pass has run on this film (rt_film_render_features)");
    if (int rc = select_device(f.device)) return rc;
    if (!f.denoised) HIP_TRY(f.planes.alloc(f.plane_pixels() * 3, f.denoised));
    if (!f.denoise_tmp && p->iterations > 1) HIP_TRY(f.planes.alloc(f.plane_pixels() * 3, f.denoise_tmp));
    // (one rank owns every row: the compact planes are the full frame)
    if (int rc = enqueue_atrous(f.pixels, f.feat_albedo, f.feat_normal, f.feat_depth, f.geometry.width, f.geometry.height, *p, f.denoised, f.denoise_tmp, f.own_stream))
        return rc;
    HIP_TRY(hipStreamSynchronize(f.own_stream));
    f.has_denoised = true;
    return RT_OK;
}

int rt_film_download_denoised(rt_film *film, double *frame_full, int width, int height)
{
    if (!film || !frame_full) return fail(RT_ERR_INVALID, "rt_film_download_denoised: null argument");
    FilmImpl &f = *F(film);
    if (width != f.geometry.width || height != f.geometry.height) return fail(RT_ERR_INVALID, "rt_film_download_denoised: frame size mismatch");
    if (!f.has_denoised) return fail(RT_ERR_STATE, "rt_film_download_denoised: nothing filtered yet (rt_film_denoise)");
    if (int rc = select_device(f.device)) return rc;
    return download_rows(f, f.denoised, 3, true, frame_full);
}

int rt_denoise_frame(int device, const double *color, const double *albedo, const double *normal, const double *depth, int width,
                     int height, const rt_denoise_params *p, double *out)
{
    if (!color || !out) return fail(RT_ERR_INVALID, "rt_denoise_frame: null colour or output");
    if (width <= 0 || height <= 0 || (int64_t)width * height >= (int64_t)1 << 31) return fail(RT_ERR_INVALID, "rt_denoise_frame: bad frame size");
    if (const char *why = denoise_params_error(p)) return fail(RT_ERR_INVALID, std::string("rt_denoise_frame: ") + why);
    if (int rc = select_device(device)) return rc;
    const size_t n = (size_t)width * (size_t)height;
    DeviceArena scratch(device);
    const double *d_color = nullptr, *d_albedo = nullptr, *d_normal = nullptr, *d_depth = nullptr;  // a guide not given stays null
    double *d_out = nullptr, *d_tmp = nullptr;
    HIP_TRY(scratch.upload(color, n * 3, d_color));
    if (albedo) HIP_TRY(scratch.upload(albedo, n * 3, d_albedo));
    if (normal) HIP_TRY(scratch.upload(normal, n * 3, d_normal));
    if (depth) HIP_TRY(scratch.upload(depth, n, d_depth));
    HIP_TRY(scratch.alloc(n * 3, d_out));
    if (p->iterations > 1) HIP_TRY(scratch.alloc(n * 3, d_tmp));
    if (int rc = enqueue_atrous(d_color, d_albedo, d_normal, d_depth, width, height, *p, d_out, d_tmp, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- ray queries ----
// everything that can be refused without a device, in the order include/rtow.h lists it
static int query_check(rt_scene *scene, const rt_query_params *p, const rt_query_rays *rays, const rt_query_hits *hits, const char *who)
{
    const std::string name(who);
    const auto mode = [&] { return p->mode != 0 && p->mode != 1 ? ": mode must be 0 (closest hit) or 1 (occlusion)" : nullptr; };
    if (int rc = batch_check(scene, p, rays, hits, name, mode)) return rc;
    if (!rays->tmin && std::isnan(p->tmin)) return fail(RT_ERR_INVALID, name + ": tmin is NaN");
    if (!rays->tmax && !(p->tmax >= (rays->tmin ? p->tmax : p->tmin))) return fail(RT_ERR_INVALID, name + ": tmax < tmin (or NaN)");
    return RT_OK;
}

int rt_scene_intersect_device(rt_scene *scene, const rt_query_params *p, const rt_query_rays *rays, const rt_query_hits *hits,
                              rt_query_stats *stats)
{
    if (int rc = query_check(scene, p, rays, hits, "rt_scene_intersect_device")) return rc;
    if (stats) *stats = rt_query_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    QueryArgs qa{};
    qa.origin = rays->origin;
    qa.direction = rays->direction;
    qa.time = rays->time;
    qa.tmin = rays->tmin;
    qa.tmax = rays->tmax;
    qa.time_all = p->time;
    qa.tmin_all = p->tmin;
    qa.tmax_all = p->tmax;
    qa.occluded = hits->occluded;
    if (p->mode == 0) {  // an occlusion query writes nothing else
        qa.t = hits->t;
        qa.normal = hits->normal;
        qa.uv = hits->uv;
        qa.albedo = hits->albedo;
        qa.leaf = hits->leaf;
        qa.front_face = hits->front_face;
        qa.material = hits->material;
    }
    qa.node_leaf_pos = dt.node_leaf_pos;
    if (int rc = device_jump_table(p->device, &qa.jump_table)) return rc;
    qa.base = xorwow_seed(p->seed, kSaltCurandDevice);
    qa.first_sequence = p->first_sequence;
    qa.count = (uint32_t)p->count;
    qa.mode = p->mode;
    hipStream_t stream = (hipStream_t)p->stream;
    // (qa by reference: the run sets qa.hit_counter between the launch that reports and the one that runs)
    const auto launch = [&](QueryKernelInfo *info) { return kBuilds[p->variant].query(dt.scene, qa, stream, info); };
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&qa.hit_counter}, 1, p->device, stream, "rt_scene_intersect_device", stats, run)) return rc;
    if (stats) {
        stats->rays = (uint64_t)p->count;
        stats->hits = run.counted[0];
    }
    return RT_OK;
}

int rt_scene_intersect(rt_scene *scene, const rt_query_params *p, const rt_query_rays *rays, const rt_query_hits *hits, rt_query_stats *stats)
{
    if (int rc = query_check(scene, p, rays, hits, "rt_scene_intersect")) return rc;
    rt_query_hits only{};  // an occlusion query writes `occluded` alone: its other outputs are neither allocated nor copied
    only.occluded = hits->occluded;
    return host_batch(scene, p, rays, p->mode == 0 ? hits : &only, stats, rt_scene_intersect_device);
}

void rt_query_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_query_params);
    out4[1] = (uint32_t)sizeof(rt_query_rays);
    out4[2] = (uint32_t)sizeof(rt_query_hits);
    out4[3] = (uint32_t)sizeof(rt_query_stats);
}

// ---- radiance queries ----
// rt_radiance_direct_params (the radiance queries with light samples, below) begins with rt_radiance_params, field for field: the
// check and the arguments of both are one template each
static_assert(sizeof(rt_radiance_direct_params) == sizeof(rt_radiance_params) + 4 * sizeof(int32_t) &&
                  offsetof(rt_radiance_direct_params, strategy) == sizeof(rt_radiance_params) &&
                  offsetof(rt_radiance_direct_params, stream) == offsetof(rt_radiance_params, stream) &&
                  offsetof(rt_radiance_direct_params, variant) == offsetof(rt_radiance_params, variant),
              "rt_radiance_direct_params: rt_radiance_params and the strategy behind it");

extern "C++" {  // (two templates among the C entry points)
// everything that can be refused without a device, in the order include/rtow.h lists it
template <class Params>
static int radiance_check(rt_scene *scene, const Params *p, const rt_radiance_rays *rays, const rt_radiance_out *out, const char *who)
{
    const std::string name(who);
    const auto paths = [&] { return p->samples < 1 || p->samples > (1 << 20) ? ": samples must be 1 .. 2^20" : p->max_depth < 0 ? ": max_depth must be >= 0" : nullptr; };
    if (int rc = batch_check(scene, p, rays, out, name, paths)) return rc;
    if (!out->radiance && !out->path_rays && !out->rng_state) return fail(RT_ERR_INVALID, name + ": every output is null");
    return RT_OK;
}

// the radiance kernels' arguments from the call's three structs
template <class Params>
static int radiance_args(const Params *p, const rt_radiance_rays *rays, const rt_radiance_out *out, RadianceArgs &ra)
{
    ra.origin = rays->origin;
    ra.direction = rays->direction;
    ra.time = rays->time;
    ra.time_all = p->time;
    ra.rng_in = rays->rng_state;
    ra.radiance = out->radiance;
    ra.path_rays = out->path_rays;
    ra.rng_out = out->rng_state;
    if (int rc = device_jump_table(p->device, &ra.jump_table)) return rc;
    ra.base = xorwow_seed(p->seed, kSaltCurandDevice);
    ra.first_sequence = p->first_sequence;
    ra.count = (uint32_t)p->count;
    ra.samples = p->samples;
    ra.max_depth = p->max_depth;
    return RT_OK;
}
}  // extern "C++"

int rt_scene_radiance_device(rt_scene *scene, const rt_radiance_params *p, const rt_radiance_rays *rays, const rt_radiance_out *out,
                             rt_radiance_stats *stats)
{
    if (int rc = radiance_check(scene, p, rays, out, "rt_scene_radiance_device")) return rc;
    if (stats) *stats = rt_radiance_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    RadianceArgs ra{};
    if (int rc = radiance_args(p, rays, out, ra)) return rc;
    hipStream_t stream = (hipStream_t)p->stream;
    // (ra by reference: the run sets ra.ray_counter between the launch that reports and the one that runs)
    const auto launch = [&](QueryKernelInfo *info) { return kBuilds[p->variant].radiance(dt.scene, ra, stream, info); };
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&ra.ray_counter}, 1, p->device, stream, "rt_scene_radiance_device", stats, run)) return rc;
    if (stats) stats->rays = run.counted[0];
    return RT_OK;
}

int rt_scene_radiance(rt_scene *scene, const rt_radiance_params *p, const rt_radiance_rays *rays, const rt_radiance_out *out,
                      rt_radiance_stats *stats)
{
    if (int rc = radiance_check(scene, p, rays, out, "rt_scene_radiance")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_radiance_device);
}

void rt_radiance_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_radiance_params);
    out4[1] = (uint32_t)sizeof(rt_radiance_rays);
    out4[2] = (uint32_t)sizeof(rt_radiance_out);
    out4[3] = (uint32_t)sizeof(rt_radiance_stats);
}

// ---- path steps ----
// everything that can be refused without a device, in the order include/rtow.h lists it
static int path_step_check(rt_scene *scene, const rt_path_step_params *p, const rt_path_step_rays *rays, const rt_path_step_out *out, const char *who)
{
    const std::string name(who);
    if (int rc = batch_check(scene, p, rays, out, name, nothing_more)) return rc;  // no parameters of its own
    if (!out->status && !out->emitted && !out->attenuation && !out->origin && !out->direction && !out->time && !out->t && !out->normal &&
        !out->front_face && !out->material && !out->rng_state)
        return fail(RT_ERR_INVALID, name + ": every output is null");
    return RT_OK;
}

int rt_scene_path_step_device(rt_scene *scene, const rt_path_step_params *p, const rt_path_step_rays *rays, const rt_path_step_out *out,
                              rt_path_step_stats *stats)
{
    if (int rc = path_step_check(scene, p, rays, out, "rt_scene_path_step_device")) return rc;
    if (stats) *stats = rt_path_step_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    StepArgs sa{};
    sa.origin = rays->origin;
    sa.direction = rays->direction;
    sa.time = rays->time;
    sa.time_all = p->time;
    sa.rng_in = rays->rng_state;
    sa.status = out->status;
    sa.emitted = out->emitted;
    sa.attenuation = out->attenuation;
    sa.origin_out = out->origin;
    sa.direction_out = out->direction;
    sa.time_out = out->time;
    sa.t = out->t;
    sa.normal = out->normal;
    sa.front_face = out->front_face;
    sa.material = out->material;
    sa.rng_out = out->rng_state;
    if (int rc = device_jump_table(p->device, &sa.jump_table)) return rc;
    sa.base = xorwow_seed(p->seed, kSaltCurandDevice);
    sa.first_sequence = p->first_sequence;
    sa.count = (uint32_t)p->count;
    hipStream_t stream = (hipStream_t)p->stream;
    // (sa by reference: the run sets sa.scattered_counter between the launch that reports and the one that runs)
    const auto launch = [&](QueryKernelInfo *info) { return kBuilds[p->variant].step(dt.scene, sa, stream, info); };
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&sa.scattered_counter}, 1, p->device, stream, "rt_scene_path_step_device", stats, run)) return rc;
    if (stats) {
        stats->rays = (uint64_t)p->count;
        stats->scattered = run.counted[0];
    }
    return RT_OK;
}

int rt_scene_path_step(rt_scene *scene, const rt_path_step_params *p, const rt_path_step_rays *rays, const rt_path_step_out *out,
                       rt_path_step_stats *stats)
{
    if (int rc = path_step_check(scene, p, rays, out, "rt_scene_path_step")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_path_step_device);
}

void rt_path_step_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_path_step_params);
    out4[1] = (uint32_t)sizeof(rt_path_step_rays);
    out4[2] = (uint32_t)sizeof(rt_path_step_out);
    out4[3] = (uint32_t)sizeof(rt_path_step_stats);
}

// ---- light sampling queries ----
// everything that can be refused without a device, in the order include/rtow.h lists it: batch_check's, the strategy before the variant
static int light_sample_check(rt_scene *scene, const rt_light_params *p, const rt_light_points *pts, const rt_light_samples *out, const char *who)
{
    const std::string name(who);
    if (int rc = batch_check(scene, p, pts, out, name, [&] { return strategy_error(p->strategy); })) return rc;
    if (!out->direction && !out->distance && !out->light && !out->pdf && !out->emitted && !out->scatter_pdf && !out->contribution && !out->rng_state)
        return fail(RT_ERR_INVALID, name + ": every output is null");
    if ((out->scatter_pdf || out->contribution) && (!pts->normal || !pts->material))
        return fail(RT_ERR_INVALID, name + ": scatter_pdf and contribution need normal and material");
    return RT_OK;
}
static int light_pdf_check(rt_scene *scene, const rt_light_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out, const char *who)
{
    const std::string name(who);
    if (int rc = batch_check(scene, p, rays, out, name, [&] { return strategy_error(p->strategy); })) return rc;
    if (!out->pdf && !out->light) return fail(RT_ERR_INVALID, name + ": every output is null");
    return RT_OK;
}

// the arguments both kernels share, and the run: `la` holds the caller's arrays already
static int run_light_kernel(rt_scene *scene, const rt_light_params *p, LightArgs &la, bool pdf_mode, const char *who, rt_light_stats *stats)
{
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    la.rows = dt.lights;
    la.cdf = dt.light_cdf[p->strategy];
    la.n_lights = dt.n_lights;
    la.time_all = p->time;
    if (int rc = device_jump_table(p->device, &la.jump_table)) return rc;
    la.base = xorwow_seed(p->seed, kSaltCurandDevice);
    la.first_sequence = p->first_sequence;
    la.count = (uint32_t)p->count;
    hipStream_t stream = (hipStream_t)p->stream;
    // (la by reference: the run sets la.valid_counter between the launch that reports and the one that runs)
    const auto launch = [&](QueryKernelInfo *info) {
        return pdf_mode ? kBuilds[p->variant].light_pdf(dt.scene, la, stream, info) : kBuilds[p->variant].light_sample(dt.scene, la, stream, info);
    };
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&la.valid_counter}, 1, p->device, stream, who, stats, run)) return rc;
    if (stats) {
        stats->points = (uint64_t)p->count;
        stats->valid = run.counted[0];
    }
    return RT_OK;
}

int rt_scene_sample_lights_device(rt_scene *scene, const rt_light_params *p, const rt_light_points *pts, const rt_light_samples *out,
                                  rt_light_stats *stats)
{
    if (int rc = light_sample_check(scene, p, pts, out, "rt_scene_sample_lights_device")) return rc;
    if (stats) *stats = rt_light_stats{};
    if (p->count == 0) return RT_OK;
    LightArgs la{};
    la.point = pts->point;
    la.normal = pts->normal;
    la.material = pts->material;
    la.time = pts->time;
    la.rng_in = pts->rng_state;
    la.direction = out->direction;
    la.distance = out->distance;
    la.light = out->light;
    la.pdf = out->pdf;
    la.emitted = out->emitted;
    la.scatter_pdf = out->scatter_pdf;
    la.contribution = out->contribution;
    la.rng_out = out->rng_state;
    return run_light_kernel(scene, p, la, false, "rt_scene_sample_lights_device", stats);
}

int rt_scene_sample_lights(rt_scene *scene, const rt_light_params *p, const rt_light_points *pts, const rt_light_samples *out, rt_light_stats *stats)
{
    if (int rc = light_sample_check(scene, p, pts, out, "rt_scene_sample_lights")) return rc;
    return host_batch(scene, p, pts, out, stats, rt_scene_sample_lights_device);
}

int rt_scene_light_pdf_device(rt_scene *scene, const rt_light_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out, rt_light_stats *stats)
{
    if (int rc = light_pdf_check(scene, p, rays, out, "rt_scene_light_pdf_device")) return rc;
    if (stats) *stats = rt_light_stats{};
    if (p->count == 0) return RT_OK;
    LightArgs la{};
    la.point = rays->origin;
    la.direction_in = rays->direction;
    la.time = rays->time;
    la.pdf = out->pdf;
    la.light = out->light;
    return run_light_kernel(scene, p, la, true, "rt_scene_light_pdf_device", stats);
}

int rt_scene_light_pdf(rt_scene *scene, const rt_light_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out, rt_light_stats *stats)
{
    if (int rc = light_pdf_check(scene, p, rays, out, "rt_scene_light_pdf")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_light_pdf_device);
}

void rt_light_abi_sizes(uint32_t out8[8])
{
    out8[0] = (uint32_t)sizeof(rt_light_params);
    out8[1] = (uint32_t)sizeof(rt_light_points);
    out8[2] = (uint32_t)sizeof(rt_light_samples);
    out8[3] = (uint32_t)sizeof(rt_light_rays);
    out8[4] = (uint32_t)sizeof(rt_light_pdf_out);
    out8[5] = (uint32_t)sizeof(rt_light_stats);
    out8[6] = (uint32_t)sizeof(rt_light_row);
    out8[7] = kLightLdsRows;
}

// ---- environment sampling ----
// everything that can be refused without a device: batch_check's, then the scene's own state
static int environment_state_check(rt_scene *scene, bool any_output, const std::string &name)
{
    if (!any_output) return fail(RT_ERR_INVALID, name + ": every output is null");
    if (!(S(scene)->flat.flags & SCENE_ENVIRONMENT)) return fail(RT_ERR_STATE, name + ": the scene has no environment (rt_scene_set_environment)");
    return RT_OK;
}
static int environment_sample_check(rt_scene *scene, const rt_environment_params *p, const rt_light_points *pts, const rt_light_samples *out, const char *who)
{
    const std::string name(who);
    if (int rc = batch_check(scene, p, pts, out, name, nothing_more)) return rc;
    const bool any = out->direction || out->distance || out->light || out->pdf || out->emitted || out->scatter_pdf || out->contribution || out->rng_state;
    if (int rc = environment_state_check(scene, any, name)) return rc;
    if ((out->scatter_pdf || out->contribution) && (!pts->normal || !pts->material))
        return fail(RT_ERR_INVALID, name + ": scatter_pdf and contribution need normal and material");
    return RT_OK;
}
static int environment_pdf_check(rt_scene *scene, const rt_environment_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out, const char *who)
{
    const std::string name(who);
    if (int rc = batch_check(scene, p, rays, out, name, nothing_more)) return rc;
    return environment_state_check(scene, out->pdf || out->light, name);
}

// the arguments both kernels share, and the run: `la` holds the caller's arrays already (run_light_kernel without a table)
static int run_environment_kernel(rt_scene *scene, const rt_environment_params *p, LightArgs &la, bool pdf_mode, const char *who, rt_light_stats *stats)
{
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    if (int rc = device_jump_table(p->device, &la.jump_table)) return rc;
    la.base = xorwow_seed(p->seed, kSaltCurandDevice);
    la.first_sequence = p->first_sequence;
    la.count = (uint32_t)p->count;
    hipStream_t stream = (hipStream_t)p->stream;
    const auto launch = [&](QueryKernelInfo *info) {
        return pdf_mode ? kBuilds[p->variant].env_pdf(dt.scene, la, stream, info) : kBuilds[p->variant].env_sample(dt.scene, la, stream, info);
    };
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&la.valid_counter}, 1, p->device, stream, who, stats, run)) return rc;
    if (stats) {
        stats->points = (uint64_t)p->count;
        stats->valid = run.counted[0];
    }
    return RT_OK;
}

int rt_scene_sample_environment_device(rt_scene *scene, const rt_environment_params *p, const rt_light_points *pts, const rt_light_samples *out,
                                       rt_light_stats *stats)
{
    if (int rc = environment_sample_check(scene, p, pts, out, "rt_scene_sample_environment_device")) return rc;
    if (stats) *stats = rt_light_stats{};
    if (p->count == 0) return RT_OK;
    LightArgs la{};
    la.point = pts->point;
    la.normal = pts->normal;
    la.material = pts->material;
    la.rng_in = pts->rng_state;
    la.direction = out->direction;
    la.distance = out->distance;
    la.light = out->light;
    la.pdf = out->pdf;
    la.emitted = out->emitted;
    la.scatter_pdf = out->scatter_pdf;
    la.contribution = out->contribution;
    la.rng_out = out->rng_state;
    return run_environment_kernel(scene, p, la, false, "rt_scene_sample_environment_device", stats);
}

int rt_scene_sample_environment(rt_scene *scene, const rt_environment_params *p, const rt_light_points *pts, const rt_light_samples *out,
                                rt_light_stats *stats)
{
    if (int rc = environment_sample_check(scene, p, pts, out, "rt_scene_sample_environment")) return rc;
    return host_batch(scene, p, pts, out, stats, rt_scene_sample_environment_device);
}

int rt_scene_environment_pdf_device(rt_scene *scene, const rt_environment_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out,
                                    rt_light_stats *stats)
{
    if (int rc = environment_pdf_check(scene, p, rays, out, "rt_scene_environment_pdf_device")) return rc;
    if (stats) *stats = rt_light_stats{};
    if (p->count == 0) return RT_OK;
    LightArgs la{};
    la.point = rays->origin;
    la.direction_in = rays->direction;
    la.pdf = out->pdf;
    la.light = out->light;
    return run_environment_kernel(scene, p, la, true, "rt_scene_environment_pdf_device", stats);
}

int rt_scene_environment_pdf(rt_scene *scene, const rt_environment_params *p, const rt_light_rays *rays, const rt_light_pdf_out *out,
                             rt_light_stats *stats)
{
    if (int rc = environment_pdf_check(scene, p, rays, out, "rt_scene_environment_pdf")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_environment_pdf_device);
}

void rt_environment_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_environment);
    out4[1] = (uint32_t)sizeof(rt_environment_params);
    out4[2] = kEnvLdsRows;
    out4[3] = 0;
}

// ---- path advances ----
// The workspace of an advance of capacity `count` (private): the workgroups' counts and offsets, the survivor flags, then one
// staging array per output, each from a multiple of 256 bytes.  Every piece grows with the count, so the total does.
struct AdvanceWorkspace {
    uint64_t block_counts, block_offsets, survivor;
    uint64_t origin, direction, time, rng_state, throughput, ray_id, t, normal, front_face, material;
    uint64_t bytes;
    uint32_t n_blocks;
};
static AdvanceWorkspace advance_workspace(int64_t count)
{
    AdvanceWorkspace w{};
    if (count <= 0) return w;
    const uint64_t n = (uint64_t)count;
    w.n_blocks = (uint32_t)((n + kAdvanceBlock - 1) / kAdvanceBlock);
    uint64_t at = 0;
    const auto piece = [&](uint64_t bytes) {
        const uint64_t here = at;
        at += (bytes + 255u) & ~(uint64_t)255u;
        return here;
    };
    w.block_counts = piece((uint64_t)w.n_blocks * sizeof(uint32_t));
    w.block_offsets = piece((uint64_t)w.n_blocks * sizeof(uint32_t));
    w.survivor = piece(n);
    w.origin = piece(n * 3 * sizeof(double));
    w.direction = piece(n * 3 * sizeof(double));
    w.time = piece(n * sizeof(double));
    w.rng_state = piece(n * 6 * sizeof(uint32_t));
    w.throughput = piece(n * 3 * sizeof(double));
    w.ray_id = piece(n * sizeof(int32_t));
    w.t = piece(n * sizeof(double));
    w.normal = piece(n * 3 * sizeof(double));
    w.front_face = piece(n);
    w.material = piece(n);
    w.bytes = at;
    return w;
}

extern "C++" {  // (two templates among the C entry points)
// what both kinds of advance refuse alike behind their parameters (rt_path_advance_* or rt_path_advance_direct_*, which begin with
// their fields): the required outputs, the aliased pairs -- `extra_in` / `extra_out` one more -- and a device call's workspace of
// at least `workspace_needed` bytes (0: the host call, which brings its own), as `measured_by` reports them
template <class Params, class Rays, class Out>
static int advance_arrays_check(const Params *p, const Rays *rays, const Out *out, const void *extra_in, const void *extra_out,
                                uint64_t workspace_needed, const char *measured_by, const std::string &name)
{
    if (!out->origin || !out->direction || !out->count) return fail(RT_ERR_INVALID, name + ": out->origin, out->direction and out->count are required");
    if (out->radiance && p->sources == 0) return fail(RT_ERR_INVALID, name + ": a radiance array of no rows (sources is 0)");
    const std::pair<const void *, const void *> pairs[] = {{rays->origin, out->origin},       {rays->direction, out->direction},
                                                           {rays->time, out->time},           {rays->rng_state, out->rng_state},
                                                           {rays->throughput, out->throughput}, {rays->ray_id, out->ray_id},
                                                           {extra_in, extra_out}};
    for (const auto &pair : pairs)
        if (pair.first && pair.first == pair.second)
            return fail(RT_ERR_INVALID, name + ": an output is the input array of the same meaning (the compaction cannot be done in place)");
    if (workspace_needed && p->count > 0 && (!p->workspace || p->workspace_bytes < workspace_needed))
        return fail(RT_ERR_INVALID, name + ": the workspace is null or smaller than " + measured_by + "(count)");
    return RT_OK;
}
}  // extern "C++"

// everything that can be refused without a device, in the order include/rtow.h lists it
static int path_advance_check(rt_scene *scene, const rt_path_advance_params *p, const rt_path_advance_rays *rays, const rt_path_advance_out *out,
                              bool device_call, const char *who)
{
    const std::string name(who);
    const auto sources = [&] { return p->sources < 0 || p->sources > ((int64_t)1 << 30) ? ": sources must be 0 .. 2^30" : nullptr; };
    if (int rc = batch_check(scene, p, rays, out, name, sources)) return rc;
    return advance_arrays_check(p, rays, out, nullptr, nullptr, device_call ? advance_workspace(p->count).bytes : 0, "rt_path_advance_workspace_bytes", name);
}

extern "C++" {
// the launch arguments of an advance from the call's three structs (rt_path_advance_* or rt_path_advance_direct_*, which begin with
// their fields) and the workspace's layout: what is asked for is staged
template <class Params, class Rays, class Out>
static void advance_args(const Params *p, const Rays *rays, const Out *out, const AdvanceWorkspace &w, AdvanceArgs &aa, AdvanceGatherArgs &ga)
{
    char *base = static_cast<char *>(p->workspace);
    const auto at = [&](uint64_t offset, const void *wanted) { return wanted ? base + offset : nullptr; };  // stage what is asked for
    aa.origin = rays->origin;
    aa.direction = rays->direction;
    aa.time = rays->time;
    aa.time_all = p->time;
    aa.rng_in = rays->rng_state;
    aa.throughput = rays->throughput;
    aa.ray_id = rays->ray_id;
    aa.alive = rays->alive;
    aa.count_in = rays->count;
    aa.radiance = out->radiance;
    aa.stage.origin = (double *)at(w.origin, out->origin);
    aa.stage.direction = (double *)at(w.direction, out->direction);
    aa.stage.time = (double *)at(w.time, out->time);
    aa.stage.rng_state = (uint32_t *)at(w.rng_state, out->rng_state);
    aa.stage.throughput = (double *)at(w.throughput, out->throughput);
    aa.stage.ray_id = (int32_t *)at(w.ray_id, out->ray_id);
    aa.stage.t = (double *)at(w.t, out->t);
    aa.stage.normal = (double *)at(w.normal, out->normal);
    aa.stage.front_face = (uint8_t *)at(w.front_face, out->front_face);
    aa.stage.material = (uint8_t *)at(w.material, out->material);
    aa.survivor = (uint8_t *)(base + w.survivor);
    aa.block_counts = (uint32_t *)(base + w.block_counts);
    aa.base = xorwow_seed(p->seed, kSaltCurandDevice);
    aa.first_sequence = p->first_sequence;
    aa.capacity = (uint32_t)p->count;
    aa.sources = (uint32_t)p->sources;
    ga.from = aa.stage;
    ga.to = AdvanceStage{out->origin, out->direction, out->time, out->rng_state, out->throughput, out->ray_id, out->t, out->normal, out->front_face, out->material};
    ga.survivor = aa.survivor;
    ga.block_offsets = (uint32_t *)(base + w.block_offsets);
    ga.capacity = aa.capacity;
}

// Runs an advance's kernels on `stream`.  stats == nullptr: enqueue, record dt.advance_done behind them and return -- whoever frees
// the tables waits for the event; otherwise timed_run, whose arguments these are, with the survivors' count for its extra word.
template <class Enqueue, class Stats>
static int run_advance(Enqueue enqueue, std::initializer_list<unsigned long long **> slots, size_t n_counters, const uint32_t *survivors,
                       DeviceTables &dt, int device, hipStream_t stream, const char *who, Stats *stats, TimedRun &run)
{
    if (!dt.advance_done) HIP_TRY(hipEventCreateWithFlags(&dt.advance_done, hipEventDisableTiming));
    if (stats) return timed_run(enqueue, slots, n_counters, survivors, device, stream, who, stats, run);
    hipError_t e = enqueue(nullptr);
    const hipError_t recorded = hipEventRecord(dt.advance_done, stream);
    if (e == hipSuccess) e = recorded;
    return e == hipSuccess ? RT_OK : hip_fail(e, who);
}
}  // extern "C++"

uint64_t rt_path_advance_workspace_bytes(int64_t count) { return advance_workspace(count > ((int64_t)1 << 30) ? (int64_t)1 << 30 : count).bytes; }

int rt_scene_path_advance_device(rt_scene *scene, const rt_path_advance_params *p, const rt_path_advance_rays *rays,
                                 const rt_path_advance_out *out, rt_path_advance_stats *stats)
{
    const char *who = "rt_scene_path_advance_device";
    if (int rc = path_advance_check(scene, p, rays, out, true, who)) return rc;
    if (stats) *stats = rt_path_advance_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    const AdvanceWorkspace w = advance_workspace(p->count);
    AdvanceArgs aa{};
    AdvanceGatherArgs ga{};
    advance_args(p, rays, out, w, aa, ga);
    if (int rc = device_jump_table(p->device, &aa.jump_table)) return rc;
    hipStream_t stream = (hipStream_t)p->stream;
    const auto three = [&](QueryKernelInfo *info) -> hipError_t {  // the call's kernels, in the stream's order (or the first one's registers)
        hipError_t e = kBuilds[p->variant].advance(dt.scene, aa, stream, info);
        if (info) return e;
        if (e == hipSuccess) e = launch_advance_scan(aa.block_counts, const_cast<uint32_t *>(ga.block_offsets), w.n_blocks, out->count, stream);
        if (e == hipSuccess) e = launch_advance_gather(ga, stream);
        return e;
    };
    TimedRun run{};
    if (int rc = run_advance(three, {&aa.stepped_counter}, 1, out->count, dt, p->device, stream, who, stats, run)) return rc;
    if (stats) {
        stats->rays = run.counted[0];
        stats->scattered = run.word;
    }
    return RT_OK;
}

int rt_scene_path_advance(rt_scene *scene, const rt_path_advance_params *p, const rt_path_advance_rays *rays, const rt_path_advance_out *out,
                          rt_path_advance_stats *stats)
{
    if (int rc = path_advance_check(scene, p, rays, out, false, "rt_scene_path_advance")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_path_advance_device);
}

void rt_path_advance_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_path_advance_params);
    out4[1] = (uint32_t)sizeof(rt_path_advance_rays);
    out4[2] = (uint32_t)sizeof(rt_path_advance_out);
    out4[3] = (uint32_t)sizeof(rt_path_advance_stats);
}

// ---- path advances with light samples ----
// The plain advance's workspace (every staging array: launch 2 reads rows the caller may not have asked for), then the staged
// densities, the shadow rays, their weighted contributions and the pending flags.
struct AdvanceDirectWorkspace {
    AdvanceWorkspace plain;
    uint64_t scatter_pdf, shadow_direction, shadow_distance, shadow_radiance, pending;
    uint64_t bytes;
};
static AdvanceDirectWorkspace advance_direct_workspace(int64_t count)
{
    AdvanceDirectWorkspace w{};
    if (count <= 0) return w;
    w.plain = advance_workspace(count);
    const uint64_t n = (uint64_t)count;
    uint64_t at = w.plain.bytes;  // (a multiple of 256)
    const auto piece = [&](uint64_t bytes) {
        const uint64_t here = at;
        at += (bytes + 255u) & ~(uint64_t)255u;
        return here;
    };
    w.scatter_pdf = piece(n * sizeof(double));
    w.shadow_direction = piece(n * 3 * sizeof(double));
    w.shadow_distance = piece(n * sizeof(double));
    w.shadow_radiance = piece(n * 3 * sizeof(double));
    w.pending = piece(n);
    w.bytes = at;
    return w;
}

// everything that can be refused without a device, in the order include/rtow.h lists it: batch_check's order, with the strategy and
// the sample switch behind the variant
static int path_advance_direct_check(rt_scene *scene, const rt_path_advance_direct_params *p, const rt_path_advance_direct_rays *rays,
                                     const rt_path_advance_direct_out *out, bool device_call, const char *who)
{
    const std::string name(who);
    const auto sources = [&] { return p->sources < 0 || p->sources > ((int64_t)1 << 30) ? ": sources must be 0 .. 2^30" : nullptr; };
    const auto lights = [&] {
        const char *why = strategy_error(p->strategy);
        return why || p->sample == 0 || p->sample == 1 ? why : ": sample must be 0 (no light samples in this call) or 1";
    };
    if (int rc = batch_check(scene, p, rays, out, name, sources, lights)) return rc;
    return advance_arrays_check(p, rays, out, rays->scatter_pdf, out->scatter_pdf, device_call ? advance_direct_workspace(p->count).bytes : 0,
                                "rt_path_advance_direct_workspace_bytes", name);
}

uint64_t rt_path_advance_direct_workspace_bytes(int64_t count)
{
    return advance_direct_workspace(count > ((int64_t)1 << 30) ? (int64_t)1 << 30 : count).bytes;
}

int rt_scene_path_advance_direct_device(rt_scene *scene, const rt_path_advance_direct_params *p, const rt_path_advance_direct_rays *rays,
                                        const rt_path_advance_direct_out *out, rt_path_advance_direct_stats *stats)
{
    const char *who = "rt_scene_path_advance_direct_device";
    if (int rc = path_advance_direct_check(scene, p, rays, out, true, who)) return rc;
    if (stats) *stats = rt_path_advance_direct_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    const AdvanceDirectWorkspace w = advance_direct_workspace(p->count);
    char *base = static_cast<char *>(p->workspace);
    AdvanceDirectArgs da{};
    AdvanceDirectGatherArgs ga{};
    advance_args(p, rays, out, w.plain, da.adv, ga.rows);
    // launch 2 reads these of every pending row, whether the caller asked for them or not
    da.adv.stage.time = (double *)(base + w.plain.time);
    da.adv.stage.rng_state = (uint32_t *)(base + w.plain.rng_state);
    da.adv.stage.ray_id = (int32_t *)(base + w.plain.ray_id);
    ga.rows.from = da.adv.stage;
    if (int rc = device_jump_table(p->device, &da.adv.jump_table)) return rc;
    da.rows = dt.lights;
    da.cdf = dt.light_cdf[p->strategy];
    da.n_lights = dt.n_lights;
    da.sample = p->sample;
    da.scatter_pdf = rays->scatter_pdf;
    da.scatter_pdf_stage = (double *)(base + w.scatter_pdf);
    da.shadow_direction = (double *)(base + w.shadow_direction);
    da.shadow_distance = (double *)(base + w.shadow_distance);
    da.shadow_radiance = (double *)(base + w.shadow_radiance);
    da.pending = (uint8_t *)(base + w.pending);
    da.node_leaf_pos = dt.node_leaf_pos;
    ga.scatter_pdf_from = da.scatter_pdf_stage;
    ga.scatter_pdf_to = out->scatter_pdf;
    // else launch 1 leaves no row pending: launch 2 is not enqueued.  (A scene whose environment is a light samples it without a table.)
    const bool shadows = (da.n_lights != 0 || (dt.scene.flags & SCENE_ENVIRONMENT_LIGHT) != 0) && da.sample != 0;
    hipStream_t stream = (hipStream_t)p->stream;
    const auto four = [&](QueryKernelInfo *info) -> hipError_t {  // the call's kernels, in the stream's order (or the registers of the first two)
        hipError_t e = kBuilds[p->variant].advance_direct(dt.scene, da, stream, info);
        if (e == hipSuccess && (shadows || info)) e = kBuilds[p->variant].advance_shadow(dt.scene, da, stream, info ? info + 1 : nullptr);
        if (info) return e;
        if (e == hipSuccess)
            e = launch_advance_scan(da.adv.block_counts, const_cast<uint32_t *>(ga.rows.block_offsets), w.plain.n_blocks, out->count, stream);
        if (e == hipSuccess) e = launch_advance_direct_gather(ga, stream);
        return e;
    };
    // the counters: rows stepped; shadow rays cast, shadow rays that reached their lamp
    TimedRun run{};
    if (int rc = run_advance(four, {&da.adv.stepped_counter, &da.shadow_counters}, 3, out->count, dt, p->device, stream, who, stats, run)) return rc;
    if (stats) {
        stats->rays = run.counted[0];
        stats->scattered = run.word;
        stats->shadow_rays = run.counted[1];
        stats->shadow_reached = run.counted[2];
        stats->shadow_vgprs = (uint32_t)run.kernel[1].vgprs;
        stats->shadow_scratch_bytes = (uint32_t)run.kernel[1].scratch_bytes;
    }
    return RT_OK;
}

int rt_scene_path_advance_direct(rt_scene *scene, const rt_path_advance_direct_params *p, const rt_path_advance_direct_rays *rays,
                                 const rt_path_advance_direct_out *out, rt_path_advance_direct_stats *stats)
{
    if (int rc = path_advance_direct_check(scene, p, rays, out, false, "rt_scene_path_advance_direct")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_path_advance_direct_device);
}

void rt_path_advance_direct_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_path_advance_direct_params);
    out4[1] = (uint32_t)sizeof(rt_path_advance_direct_rays);
    out4[2] = (uint32_t)sizeof(rt_path_advance_direct_out);
    out4[3] = (uint32_t)sizeof(rt_path_advance_direct_stats);
}

// ---- radiance queries with light samples ----
// everything that can be refused without a device, in the order include/rtow.h lists it: rt_scene_radiance's, then the strategy
static int radiance_direct_check(rt_scene *scene, const rt_radiance_direct_params *p, const rt_radiance_rays *rays, const rt_radiance_out *out,
                                 const char *who)
{
    if (int rc = radiance_check(scene, p, rays, out, who)) return rc;
    if (const char *why = strategy_error(p->strategy)) return fail(RT_ERR_INVALID, std::string(who) + why);
    return RT_OK;
}

int rt_scene_radiance_direct_device(rt_scene *scene, const rt_radiance_direct_params *p, const rt_radiance_rays *rays, const rt_radiance_out *out,
                                    rt_radiance_direct_stats *stats)
{
    const char *who = "rt_scene_radiance_direct_device";
    if (int rc = radiance_direct_check(scene, p, rays, out, who)) return rc;
    if (stats) *stats = rt_radiance_direct_stats{};
    if (p->count == 0) return RT_OK;
    SceneImpl &s = *S(scene);
    if (int rc = rt_scene_upload(scene, p->device)) return rc;  // (selects the device)
    DeviceTables &dt = *s.device[p->device];
    RadianceDirectArgs da{};
    if (int rc = radiance_args(p, rays, out, da.rad)) return rc;
    da.rows = dt.lights;
    da.cdf = dt.light_cdf[p->strategy];
    da.n_lights = dt.n_lights;
    da.node_leaf_pos = dt.node_leaf_pos;
    hipStream_t stream = (hipStream_t)p->stream;
    const auto launch = [&](QueryKernelInfo *info) { return kBuilds[p->variant].radiance_direct(dt.scene, da, stream, info); };
    // the counters: path searches; shadow rays cast, shadow rays that reached their lamp
    TimedRun run{};
    if (int rc = run_lane_kernel(launch, {&da.rad.ray_counter, &da.shadow_counters}, 3, p->device, stream, who, stats, run)) return rc;
    if (stats) {
        stats->rays = run.counted[0];
        stats->shadow_rays = run.counted[1];
        stats->shadow_reached = run.counted[2];
    }
    return RT_OK;
}

int rt_scene_radiance_direct(rt_scene *scene, const rt_radiance_direct_params *p, const rt_radiance_rays *rays, const rt_radiance_out *out,
                             rt_radiance_direct_stats *stats)
{
    if (int rc = radiance_direct_check(scene, p, rays, out, "rt_scene_radiance_direct")) return rc;
    return host_batch(scene, p, rays, out, stats, rt_scene_radiance_direct_device);
}

void rt_radiance_direct_abi_sizes(uint32_t out4[4])
{
    out4[0] = (uint32_t)sizeof(rt_radiance_direct_params);
    out4[1] = (uint32_t)sizeof(rt_radiance_rays);
    out4[2] = (uint32_t)sizeof(rt_radiance_out);
    out4[3] = (uint32_t)sizeof(rt_radiance_direct_stats);
}

int rt_render(rt_scene *scene, const rt_render_params *params, double *frame, rt_render_stats *stats)
{
    if (!scene || !params || !frame) return fail(RT_ERR_INVALID, "rt_render: null argument");
    rt_film *film = rt_film_create(params->device, params->width, params->height, params->stripe_rows > 0 ? params->stripe_rows : 8,
                                   params->rank, params->world_size > 0 ? params->world_size : 1);
    if (!film) return std::strstr(rt_last_error(), "no HIP device") ? RT_ERR_NO_DEVICE : RT_ERR_HIP;
    rt_render_params p = *params;
    if (p.stripe_rows <= 0) p.stripe_rows = 8;
    if (p.world_size <= 0) p.world_size = 1;
    int rc = rt_render_launch(scene, film, &p);
    if (rc == RT_OK) rc = rt_render_finish(scene, film, stats);
    if (rc == RT_OK) rc = rt_film_download(film, frame, p.width, p.height);
    rt_film_destroy(film);
    return rc;
}

} // extern "C"
