// render.hip -- the gfx950 path-tracing megakernel and the RNG seeding kernel.
//
// Replaces the reference's RenderInit + Render kernels (R/kernel.cu:110-154) and everything they
// inline: Camera::GetRay (R/Camera.h:76-85), RayColor (R/kernel.cu:65-98), BvhNode::Hit
// (R/BvhNode.h:101-158), the primitive / instance / medium Hit functions, Material::Scatter/Emitted
// and Texture::Value.  Not a translation: one lane owns one pixel and runs a flat
// "one ray segment per iteration" loop with path regeneration (a lane whose path ends starts its
// pixel's next sample in the same iteration), virtual dispatch is tag dispatch over the SoA tables
// of flat_scene.h, the BVH is walked stacklessly through escape links with its nodes staged in LDS,
// a list-of-spheres world is scanned with wave-uniform (scalar-path) primitive rows while the rare
// sqrt/divide root work is deferred to a per-lane LDS queue, hit records are built once per bounce
// from (t, primitive) instead of on every accepted candidate, and sphere UVs are computed only when
// an image texture will read them.  Each of these is result-preserving: see DESIGN.md.
//
// This file is compiled twice: RT_STRICT=1 with -ffp-contract=off (no FMA; bit-comparable with the
// CPU oracle) and RT_STRICT=0 with the default contraction (fast variant) -- and each of those in two groups of
// instantiations (RT_GROUP), because they want different code generation: group 0 (sphere-list and primitive-BVH
// kernels, seeding, dispatch) with the compiler's defaults, group 1 (every kernel with composite leaves, media or table
// textures) with machine-level loop-invariant code motion off.  There LICM hoists the libm polynomial coefficients and
// other constants of rarely executed code (log, sin, acos, atan2) out of the main loop into ~100 VGPRs and the register
// allocator then spills them: 520 B/lane of scratch in the deep general kernel, 80 B without (C5 +10 %); the tight
// primitive walk loses 5-7 % the same way, hence the split.
// Both groups are compiled once more with RT_ADAPT=1: those objects hold the Adaptive<> forms of the group's instantiations
// (adaptive sampling, adaptive_rule.h) and nothing else, so that the objects without it hold exactly the kernels they always held.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "flat_scene.h"
#include "launch_plan.h"
#include "primary_cull_rule.h"
#include "scan_window_rule.h"
#include "render_iface.h"
#include "rng.h"

#ifndef RT_STRICT
#define RT_STRICT 1
#endif
#ifndef RT_GROUP
#define RT_GROUP 0
#endif
#ifndef RT_ADAPT  // 1: this translation unit holds the Adaptive<> instantiations of its group and nothing else
#define RT_ADAPT 0
#endif
#ifndef RT_FEATURES  // 1: this translation unit holds the first-hit feature kernels (feature_kernel) and nothing else
#define RT_FEATURES 0
#endif
#ifndef RT_QUERY  // 1: this translation unit holds the ray-query kernels (query_kernel) and nothing else
#define RT_QUERY 0
#endif
#ifndef RT_RADIANCE  // 1: this translation unit holds the radiance-query kernels (radiance_kernel) and nothing else
#define RT_RADIANCE 0
#endif
#ifndef RT_STEP  // 1: this translation unit holds the path-step kernels (step_kernel) and nothing else
#define RT_STEP 0
#endif
#ifndef RT_ADVANCE  // 1: this translation unit holds the path-advance kernels (advance_kernel) and nothing else
#define RT_ADVANCE 0
#endif
#ifndef RT_LIGHTS  // 1: this translation unit holds the light sampling kernels (light_sample_kernel, light_pdf_kernel) and nothing else
#define RT_LIGHTS 0
#endif
#ifndef RT_ADVANCE_DIRECT  // 1: this translation unit holds the kernels of a path advance with light samples (advance_direct_kernel, shadow_kernel) and nothing else
#define RT_ADVANCE_DIRECT 0
#endif
#ifndef RT_RADIANCE_DIRECT  // 1: this translation unit holds the radiance-query kernels with light samples (radiance_direct_kernel) and nothing else
#define RT_RADIANCE_DIRECT 0
#endif
#ifndef RT_FILM_DIRECT  // 1: this translation unit holds the frame kernels with light samples (film_direct_kernel) and nothing else
#define RT_FILM_DIRECT 0
#endif
#ifndef RT_AFFINE  // 1: this translation unit compiles the general affine chain step (rt_transform) into its chain walks; its launchers
#define RT_AFFINE 0  // carry the suffix _x and serve the scenes with SCENE_AFFINE.  0: chains hold Translate / RotateY only, the code without it
#endif
#ifndef RT_MOVING  // 1: the second pass of an RT_AFFINE unit over this file (its last lines include it once more): everything again in
#define RT_MOVING 0  // namespace rtow::moving with the moving chain step (rt_moving_transform) compiled into the chain walks; those launchers
#endif               // carry the suffix _xm and serve the scenes with SCENE_MOVING.  0: the walks hold no such branch
// the lane-per-ray units: one lane per pixel, ray or point, no persistent waves (film_direct_kernel alone is persistent: its lanes take pixels from a queue)
#define RT_LANE_UNIT (RT_FEATURES || RT_QUERY || RT_RADIANCE || RT_STEP || RT_ADVANCE || RT_LIGHTS || RT_ADVANCE_DIRECT || RT_RADIANCE_DIRECT || RT_FILM_DIRECT)

namespace rtow {
#if RT_MOVING
namespace moving {
#endif
#if RT_AFFINE
inline namespace affine {
#endif
namespace {
constexpr bool kAffineUnit = RT_AFFINE != 0;
constexpr bool kMovingUnit = RT_MOVING != 0;

// Kernel specialisation.  One source, a few instantiations; the host picks by what the scene contains so
// that a scene never pays registers or code for features it does not use:
//   WORLD      0 = BvhNode world (threaded, nodes staged in LDS), 1 = HittableList world (uniform scan),
//              2 = HittableList of static spheres only (config C2: scalar-fed discriminant scan + LDS queue)
//   COMPOSITE  instances / boxes / lists / media may appear as leaves
//   RICH       Perlin-noise or image textures may appear
//   BATCH      BVH world with composite leaves: the leaf phase runs one kind of leaf at a time (deep trees, see walk_leaf_pass)
//   NESTED     REF_TREE leaves may appear: composites kept as the reference's object tree (tree_hit)
//   BLOCK      threads per workgroup.  256 (four waves) everywhere except the deep general kernel, which runs ONE workgroup of
//              768 threads per CU -- three waves per SIMD as before, but one copy of the scene tables in the CU's 160 KB of LDS
//              instead of three in 52 KB each: besides the node rows, the box rows and the sphere table fit as well
//   FAST       primitive-only BVH world walked through the library's own SAH tree, near child first (flat_scene.h FastNodeRec)
//              (with COMPOSITE and BATCH: the segmented walk of a composite world, Traits::SEG)
//   GROUPED    list scan with the leaves of every ray dealt to several lanes (scan_leaves_grouped): launches with pixels_per_wave < 64
constexpr int kBigBlock = 768;  // workgroups this large run one per CU with the scene tables in (nearly) all of its LDS
template <int WORLD_, bool COMPOSITE_, bool RICH_, int MIN_WAVES_ = 1, bool MEDIA_ = COMPOSITE_, bool BATCH_ = false, bool NESTED_ = false,
          int BLOCK_ = 256, bool FAST_ = false, bool GROUPED_ = false>
struct Traits {
    static constexpr bool GROUPED = GROUPED_ && WORLD_ == 1 && !MEDIA_ && !NESTED_;
    // list scan over instances / boxes compiled for five waves per SIMD (C4, TListInstances5): the path state the scan does not touch
    // -- pixel sum, throughput, emitted light, RNG, pixel counters -- waits in LDS while the leaves are tested (park_* in
    // render_kernel), so that 96 registers are nearly enough (at four waves the same parking costs 2.5 %: measured, not used)
    static constexpr bool PARK = WORLD_ == 1 && COMPOSITE_ && !RICH_ && !MEDIA_ && !NESTED_ && !GROUPED_ && MIN_WAVES_ >= 5;
    // segmented walk (flat_scene.h FastOrder / SegMedium): the library's tree over the surface leaves of a composite BVH world,
    // walked once per run of leaves between two media; kind-batched leaf phases, one 768-thread workgroup per CU
    static constexpr bool SEG = FAST_ && COMPOSITE_ && BATCH_ && WORLD_ == 0 && BLOCK_ >= kBigBlock;
    static constexpr bool FAST = FAST_ && !COMPOSITE_ && WORLD_ == 0;
    // kernels that can be launched with heavy / light pixel classes (RenderArgs::heavy_list): for the others the serving code folds away
    static constexpr bool ROLES = WORLD_ == 2 || (FAST_ && WORLD_ == 0 && BLOCK_ >= kBigBlock) || (COMPOSITE_ && BATCH_ && WORLD_ == 0 && BLOCK_ >= kBigBlock);
    static constexpr int BLOCK = BLOCK_;
    static constexpr bool NESTED = NESTED_ && COMPOSITE_;
    static constexpr bool BATCH = BATCH_ && COMPOSITE_ && WORLD_ == 0;
    static constexpr bool MEDIA = MEDIA_;  // ConstantMedium leaves may appear (needs COMPOSITE)
    static constexpr int MIN_WAVES = MIN_WAVES_;  // waves per SIMD the register allocator must leave room for
    static constexpr int WORLD = WORLD_;
    static constexpr bool COMPOSITE = COMPOSITE_;
    static constexpr bool RICH = RICH_;
    static constexpr bool ADAPTIVE = false;
};
// The same instantiation with adaptive sampling (adaptive_rule.h): a type of its own, so that a film without it launches
// exactly the kernels it always did.  Three more registers of path state (q, and the samples the pixel had before the
// launch), the rule at the end of a sample, the per-pixel planes where a pixel is taken up and laid down.
template <class T>
struct Adaptive : T {
    static constexpr bool ADAPTIVE = true;
};
// the instantiation U as the launch that chose T wants it: adaptive or not
template <class T, class U>
struct LikeImpl { using type = U; };
template <class T, class U>
struct LikeImpl<Adaptive<T>, U> { using type = Adaptive<U>; };
template <class T, class U>
using Like = typename LikeImpl<T, U>::type;

struct Vec {
    double x, y, z;
};
struct Ray {
    Vec o, d;
    double tm;
};
struct HitInfo {
    double t;
    uint32_t ref;  // primitive (or medium) that won
    uint32_t obj;  // enclosing composite object, or kNone
};
struct Surface {
    Vec p, n;
    double u, v;
    uint32_t mat;
    bool front;
};

// BVH nodes as the traversal sees them: 72-byte rows in LDS (or the global 64-byte table when they do not fit).
// The LDS copy is addressed straight off the __shared__ symbol (see lds_node_*), never through generic pointers:
// a pointer that may be LDS or global makes the compiler emit flat loads plus aperture arithmetic per access.
struct NodeView {
    const BvhNodeRec *global;
    uint32_t n;      // number of staged nodes (plane stride)
    bool in_lds;
};

#define DEV __device__ __forceinline__
#define RT_LDS __attribute__((address_space(3)))  // pointers typed for LDS: loads through them are ds_read, never flat

extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

// BVH nodes in LDS: one 72-byte row per node -- six doubles (xlo, xhi, ylo, yhi, zlo, zhi), three words (a, b, escape),
// one word of padding.  One base address per visit and immediate offsets (ds_read2_b64) instead of one address per
// field; the odd multiple of 8 bytes spreads the rows of 64 lanes standing on 64 different nodes over 32 bank
// positions (64-byte rows would fall on 4).
constexpr uint32_t kLdsNodeBytes = 72;
DEV double lds_node_f64(uint32_t, uint32_t field, uint32_t node)
{
    return reinterpret_cast<const double *>(lds_raw + __umul24(node, kLdsNodeBytes))[field];  // node < 2^24: 24-bit multiply
}
DEV uint32_t lds_node_u32(uint32_t, uint32_t word, uint32_t node)
{
    return reinterpret_cast<const uint32_t *>(lds_raw + __umul24(node, kLdsNodeBytes) + 48u)[word];
}

// Scene tables are immutable for the whole launch.  Reading them through the constant address space tells
// the compiler so: a wave-uniform row then always comes through the scalar cache into SGPRs, even though the
// kernel stores pixels inside its main loop (which defeats alias analysis for ordinary global loads).
#define RT_CONST __attribute__((address_space(4)))

// Small tables staged in LDS (DeviceScene::lds_*): a row by byte offset off the same symbol.
template <class R>
DEV R lds_row(uint32_t byte_off, uint32_t idx)
{
    return *reinterpret_cast<const R *>(lds_raw + byte_off + idx * (uint32_t)sizeof(R));
}
// Tables are immutable for the whole launch: read through the constant address space, a wave-uniform index (list
// scans) then comes through the scalar cache, a per-lane one as an ordinary (invariant) vector load.
template <class R>
DEV R const_row(const R *table, uint32_t i)
{
    static_assert(sizeof(R) % 8 == 0, "rows are whole quadwords");
    const RT_CONST uint64_t *src = (const RT_CONST uint64_t *)(uintptr_t)(table + i);
    union {
        R row;
        uint64_t w[sizeof(R) / 8];
    } u;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(R) / 8; k++) u.w[k] = src[k];
    return u.row;
}
// The same through a pointer typed for the LDS address space, for call sites that choose between the LDS copy and the global
// table at run time: two loads through generic pointers get merged into one flat load through a selected pointer.
template <class R>
DEV R lds_row_typed(uint32_t byte_off, uint32_t idx)
{
    static_assert(sizeof(R) % 8 == 0, "rows are whole quadwords");
    const RT_LDS uint64_t *src = (const RT_LDS uint64_t *)(lds_raw + byte_off + idx * (uint32_t)sizeof(R));
    union {
        R row;
        uint64_t w[sizeof(R) / 8];
    } u;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(R) / 8; k++) u.w[k] = src[k];
    return u.row;
}
DEV MSphereGeom get_msphere(const DeviceScene &sc, uint32_t i) { return sc.lds_mspheres != kNone ? lds_row_typed<MSphereGeom>(sc.lds_mspheres, i) : sc.mspheres[i]; }
DEV SphereAux get_msphere_aux(const DeviceScene &sc, uint32_t i) { return sc.lds_msphere_aux != kNone ? lds_row_typed<SphereAux>(sc.lds_msphere_aux, i) : sc.msphere_aux[i]; }
DEV SphereAux get_sphere_aux(const DeviceScene &sc, uint32_t i) { return sc.lds_sphere_aux != kNone ? lds_row_typed<SphereAux>(sc.lds_sphere_aux, i) : sc.sphere_aux[i]; }
DEV SphereGeom get_sphere_typed(const DeviceScene &sc, uint32_t i) { return sc.lds_spheres_tab != kNone ? lds_row_typed<SphereGeom>(sc.lds_spheres_tab, i) : sc.spheres[i]; }
DEV AAQuad get_quad_aa(const DeviceScene &sc, uint32_t i) { return sc.lds_quad_aa != kNone ? lds_row<AAQuad>(sc.lds_quad_aa, i) : const_row(sc.quad_aa, i); }
DEV BoxRec get_box(const DeviceScene &sc, uint32_t i) { return sc.lds_boxes != kNone ? lds_row<BoxRec>(sc.lds_boxes, i) : const_row(sc.boxes, i); }
DEV ObjectRec get_object(const DeviceScene &sc, uint32_t i) { return sc.lds_objects != kNone ? lds_row<ObjectRec>(sc.lds_objects, i) : const_row(sc.objects, i); }
DEV Xform get_xform(const DeviceScene &sc, uint32_t i) { return sc.lds_xforms != kNone ? lds_row<Xform>(sc.lds_xforms, i) : const_row(sc.xforms, i); }
DEV SphereGeom get_sphere(const DeviceScene &sc, uint32_t i) { return sc.lds_spheres_tab != kNone ? lds_row<SphereGeom>(sc.lds_spheres_tab, i) : sc.spheres[i]; }
DEV GroupBox get_group_box(const DeviceScene &sc, uint32_t i) { return sc.lds_group_boxes != kNone ? lds_row<GroupBox>(sc.lds_group_boxes, i) : sc.group_boxes[i]; }
DEV MediumRec get_medium(const DeviceScene &sc, uint32_t i) { return sc.lds_media != kNone ? lds_row<MediumRec>(sc.lds_media, i) : const_row(sc.media, i); }
DEV bool material_needs_uv(const DeviceScene &sc, uint32_t i)
{
    if (sc.lds_materials != kNone)
        return *(const RT_LDS uint32_t *)(lds_raw + sc.lds_materials + i * (uint32_t)sizeof(MaterialRec) + (uint32_t)offsetof(MaterialRec, needs_uv)) != 0;
    return sc.materials[i].needs_uv != 0;
}

template <class T>
DEV const RT_CONST double *const_doubles(const T *p)
{
    return (const RT_CONST double *)(uintptr_t)p;
}
DEV SphereGeom load_sphere_row(const SphereGeom *table, uint32_t k)
{
    const RT_CONST double *p = const_doubles(table + k);
    return SphereGeom{p[0], p[1], p[2], p[3]};
}

DEV Vec mk(double x, double y, double z) { return Vec{x, y, z}; }
DEV Vec operator+(Vec a, Vec b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEV Vec operator-(Vec a, Vec b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEV Vec operator-(Vec a) { return mk(-a.x, -a.y, -a.z); }
DEV Vec operator*(Vec a, Vec b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
DEV Vec operator*(double t, Vec a) { return mk(t * a.x, t * a.y, t * a.z); }
DEV double dot(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DEV Vec cross(Vec u, Vec v) { return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }
DEV double length_sq(Vec a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
DEV double length(Vec a) { return sqrt(length_sq(a)); }
DEV Vec over(Vec a, double t) { return (1 / t) * a; }  // R/Vec3.h:103-106: v / t is (1/t) * v
DEV Vec unit(Vec a) { return over(a, length(a)); }
DEV Vec at(const Ray &r, double t) { return r.o + t * r.d; }
DEV Vec reflect(Vec v, Vec n) { return v - (2.0 * dot(v, n)) * n; }  // R/Vec3.h:127-130
DEV Vec refract(Vec uv, Vec n, double eta)                            // R/Vec3.h:132-141
{
    double ct = fmin(dot(-uv, n), 1.0);
    Vec perp = eta * (uv + ct * n);
    Vec par = (-sqrt(fabs(1.0 - length_sq(perp)))) * n;
    return perp + par;
}

// ------------------------------------------------------------------------------------------------
// primitive tests.  Each returns the accepted t exactly as the reference's Hit would set rec.T.
// ------------------------------------------------------------------------------------------------
// Root selection of R/Sphere.h:36-60 given b, disc (> 0) and a.  The second root is only evaluated when
// the first is at or below tmin: if the first root is >= tmax so is the second (a > 0, s >= 0, and
// division by a is monotone), so the reference's second test cannot pass there either.
DEV bool sphere_roots(double b, double disc, double a, double tmin, double tmax, double &t_out)
{
    double s = sqrt(disc);
    double t = (-b - s) / a;
    if (t < tmax) {
        if (t > tmin) {
            t_out = t;
            return true;
        }
        t = (-b + s) / a;
        if (t < tmax && t > tmin) {
            t_out = t;
            return true;
        }
    }
    return false;
}

// R/Sphere.h:28-60 (also MovingSphere.h:54-86): strict interval, disc > 0, first root then second.
DEV bool sphere_test(Vec oc, Vec d, double a, double r2, double tmin, double tmax, double &t_out)
{
    double b = dot(oc, d);
    double c = dot(oc, oc) - r2;
    double disc = b * b - a * c;
    if (disc > 0.0) {
        // Both roots are <= 0 when the origin is outside (c > 0) and the sphere lies behind (b > 0):
        // -b - s < 0, and s = sqrt(b*b - a*c) <= |b| in fp64 because a*c > 0, so -b + s <= 0.  With
        // tmin >= 0 neither can pass `temp > tmin`; skipping the sqrt/divides changes nothing.
        if (tmin >= 0.0 && b > 0.0 && c > 0.0) return false;
        return sphere_roots(b, disc, a, tmin, tmax, t_out);
    }
    return false;
}

// R/Quad.h:52-99: inclusive interval, inclusive unit square.  tri: the interior rule the comment above Quad::IsInterior
// (R/Quad.h:86-88) names for a triangle, inclusive like the quad's: 0 <= alpha, 0 <= beta, fl(alpha + beta) <= 1.  Plane, t,
// alpha and beta are the quad's own, so a triangle (Q, u, v) is hit exactly where the quad (Q, u, v) is hit with such alpha, beta.
// Two forms of that decision give the same answers (the quad's rule is a necessary part of the triangle's: alpha, beta >= 0 and
// fl(alpha + beta) <= 1 imply alpha, beta <= 1): the quad's rule as it was with one more branch behind it for a triangle row, or a
// select between the two upper bounds.  Which one the register allocator takes better differs by kernel, and both were timed
// against the parent commit (profiles/r16_kernel_table.txt, profiles/r16_triangle_ab.txt): the render kernels keep their frame
// times with the branch (the select costs the media kernel of scene 8 3 %), the lane-per-ray kernels of the feature pass and the
// queries keep their registers with the select (the branch takes the radiance kernel of list worlds from 168 to 170 VGPRs, from
// three waves per SIMD to two, 35 % on scene 7).  A third form, a switch case of its own in quad_test_at, cost most kernels spills.
#define RT_PLANAR_SELECT (RT_FEATURES || RT_QUERY || RT_RADIANCE || RT_STEP || RT_ADVANCE || RT_ADVANCE_DIRECT || RT_RADIANCE_DIRECT || RT_FILM_DIRECT)
DEV bool quad_test(const QuadGeom &q, bool tri, const Ray &r, double tmin, double tmax, double &t_out)
{
    Vec n = mk(q.nx, q.ny, q.nz);
    double denom = dot(n, r.d);
    if (fabs(denom) < 1e-8) return false;
    double t = (q.d - dot(n, r.o)) / denom;
    if (t < tmin || t > tmax) return false;
    Vec ph = at(r, t) - mk(q.qx, q.qy, q.qz);
    Vec w = mk(q.wx, q.wy, q.wz);
    double alpha = dot(w, cross(ph, mk(q.vx, q.vy, q.vz)));
    double beta = dot(w, cross(mk(q.ux, q.uy, q.uz), ph));
#if RT_PLANAR_SELECT
    const bool below = tri ? alpha + beta <= 1.0 : (alpha <= 1.0 && beta <= 1.0);
    if (!(0.0 <= alpha && 0.0 <= beta && below)) return false;  // (a NaN rejects)
#else
    if (!(0.0 <= alpha && alpha <= 1.0) || !(0.0 <= beta && beta <= 1.0)) return false;
    if (tri) {
        if (!(alpha + beta <= 1.0)) return false;  // (a NaN was rejected above)
    }
#endif
    t_out = t;
    return true;
}

// Axis-aligned quads (AAQuad, flat_scene.h): the same t, alpha and beta as quad_test, without the terms that are exact zeros.
template <int K>
DEV double comp(const Vec &v)
{
    return K == 0 ? v.x : (K == 1 ? v.y : v.z);
}
template <int A>
DEV bool aa_plane(double na, double d, const Ray &r, double tmin, double tmax, double &t)
{
    double denom = na * comp<A>(r.d);
    t = (d - na * comp<A>(r.o)) / denom;
    return !(fabs(denom) < 1e-8) && !(t < tmin || t > tmax);
}
template <int P, int Q>
DEV bool aa_inside(double wa, double qp, double qq, double ku, double kv, const Ray &r, double t)
{
    double php = (comp<P>(r.o) + t * comp<P>(r.d)) - qp;
    double phq = (comp<Q>(r.o) + t * comp<Q>(r.d)) - qq;
    double alpha = wa * (php * kv);
    double beta = wa * (ku * phq);
    return (0.0 <= alpha && alpha <= 1.0) && (0.0 <= beta && beta <= 1.0);
}
template <int A, int P>
DEV bool aa_quad_test(const AAQuad &q, const Ray &r, double tmin, double tmax, double &t_out)
{
    double t;
    if (!aa_plane<A>(q.na, q.d, r, tmin, tmax, t)) return false;
    if (!aa_inside<P, 3 - A - P>(q.wa, q.qp, q.qq, q.ku, q.kv, r, t)) return false;
    t_out = t;
    return true;
}
DEV bool quad_test_at(const DeviceScene &sc, uint32_t idx, const Ray &r, double tmin, double tmax, double &t)
{
    const AAQuad q = get_quad_aa(sc, idx);
    switch (q.code) {
    case 1 + 3 * 0 + 1: return aa_quad_test<0, 1>(q, r, tmin, tmax, t);
    case 1 + 3 * 0 + 2: return aa_quad_test<0, 2>(q, r, tmin, tmax, t);
    case 1 + 3 * 1 + 0: return aa_quad_test<1, 0>(q, r, tmin, tmax, t);
    case 1 + 3 * 1 + 2: return aa_quad_test<1, 2>(q, r, tmin, tmax, t);
    case 1 + 3 * 2 + 0: return aa_quad_test<2, 0>(q, r, tmin, tmax, t);
    case 1 + 3 * 2 + 1: return aa_quad_test<2, 1>(q, r, tmin, tmax, t);
    default: return quad_test(const_row(sc.quads, idx), q.code == kQuadTriangle, r, tmin, tmax, t);  // (flat_scene.h kQuadTriangle)
    }
}

// MakeBox (R/Instance.h:166-184) as HittableList::Hit sees it (R/HittableList.h:39-57): six faces in list order
// against one running closest-so-far.  The six plane distances do not depend on each other, so they are evaluated
// together (six divides in flight instead of one after another); the interior tests then run in list order.
//
// Interior test of a face with in-plane axes p, q.  R/Quad.h:86-96 accepts when alpha and beta are in [0, 1], where
// (AAQuad) alpha = fl(wa * fl(fl(P[p] - Q[p]) * kv)) = (P[p] - Q[p]) / u[p] * (1 + e), |e| < 2^-49, P the hit point
// as computed.  The host has checked (box_of_six) that Q[p] is mn[p] with u[p] = fl(mx[p] - mn[p]), or mx[p] with the
// negated extent.  With m = 2^-30 (|mn[p]| + |mx[p]|):
//   mn[p] + m <= P[p] <= mx[p] - m  =>  2^-30 <= (P[p] - Q[p]) / u[p] <= 1 - 2^-31  =>  alpha in [0, 1] for certain;
//   P[p] < mn[p] - m or P[p] > mx[p] + m  =>  alpha < 0 or alpha > 1 for certain;
// the same for beta along q.  Only a hit point inside the 2m sliver around an edge needs alpha / beta themselves.
DEV bool box_closest(const DeviceScene &sc, const BoxRec &bx, const Ray &r, double tmin, double tmax, double &t_best,
                     uint32_t &ref_best)
{
    double t[6];
    bool ok[6];
    ok[0] = aa_plane<2>(bx.na[0], bx.d[0], r, tmin, tmax, t[0]);  // front
    ok[1] = aa_plane<0>(bx.na[1], bx.d[1], r, tmin, tmax, t[1]);  // right
    ok[2] = aa_plane<2>(bx.na[2], bx.d[2], r, tmin, tmax, t[2]);  // back
    ok[3] = aa_plane<0>(bx.na[3], bx.d[3], r, tmin, tmax, t[3]);  // left
    ok[4] = aa_plane<1>(bx.na[4], bx.d[4], r, tmin, tmax, t[4]);  // top
    ok[5] = aa_plane<1>(bx.na[5], bx.d[5], r, tmin, tmax, t[5]);  // bottom
    const Vec mn = mk(bx.mn[0], bx.mn[1], bx.mn[2]), mx = mk(bx.mx[0], bx.mx[1], bx.mx[2]);
    const double k30 = 9.313225746154785e-10;  // 2^-30
    const Vec m = mk(k30 * (fabs(mn.x) + fabs(mx.x)), k30 * (fabs(mn.y) + fabs(mx.y)), k30 * (fabs(mn.z) + fabs(mx.z)));
    // (the four bounds from a host-made table through scalar loads instead: measured 1-3 % slower, four and five waves per SIMD)
    const Vec in_lo = mn + m, in_hi = mx - m, out_lo = mn - m, out_hi = mx + m;
    const uint32_t quad_first = bx.quad_first;
    double closest = tmax;
    bool any = false;
#define RT_BOX_FACE(k, P, Q)                                                                                            \
    {                                                                                                                   \
        /* straight-line: every lane evaluates every face (selects); only the sliver case branches */                   \
        const double pp = comp<P>(r.o) + t[k] * comp<P>(r.d), pq = comp<Q>(r.o) + t[k] * comp<Q>(r.d);                  \
        bool accept = pp >= comp<P>(in_lo) && pp <= comp<P>(in_hi) && pq >= comp<Q>(in_lo) && pq <= comp<Q>(in_hi);     \
        const bool outside = pp < comp<P>(out_lo) || pp > comp<P>(out_hi) || pq < comp<Q>(out_lo) || pq > comp<Q>(out_hi); \
        const bool live = ok[k] && !(t[k] > closest);                                                                   \
        if (live && !accept && !outside) {                                                                              \
            const AAQuad f = get_quad_aa(sc, quad_first + k);                                                           \
            accept = aa_inside<P, Q>(f.wa, f.qp, f.qq, f.ku, f.kv, r, t[k]);                                            \
        }                                                                                                               \
        const bool take = live && accept;                                                                               \
        closest = take ? t[k] : closest;                                                                                \
        ref_best = take ? make_ref(REF_QUAD, quad_first + k) : ref_best;                                                \
        any = any || take;                                                                                              \
    }
    RT_BOX_FACE(0, 0, 1)
    RT_BOX_FACE(1, 2, 1)
    RT_BOX_FACE(2, 0, 1)
    RT_BOX_FACE(3, 2, 1)
    RT_BOX_FACE(4, 0, 2)
    RT_BOX_FACE(5, 0, 2)
#undef RT_BOX_FACE
    t_best = closest;
    return any;
}

// unit_time: every row has time0 = 0 and time1 - time0 = 1, so (tm - 0) / 1 == tm exactly and the divide is skipped
DEV Vec msphere_center(const MSphereGeom &g, double tm, bool unit_time = false)  // R/MovingSphere.h:51-52
{
    double frac = unit_time ? tm : (tm - g.t0) / g.dt;
    return mk(g.c0x, g.c0y, g.c0z) + frac * mk(g.dcx, g.dcy, g.dcz);
}

DEV bool prim_test(const DeviceScene &sc, uint32_t ref, const Ray &r, double a, double tmin, double tmax, double &t)
{
    uint32_t idx = ref & kRefIndexMask;
    switch (ref >> kRefShift) {
    case REF_SPHERE: {
        SphereGeom g = sc.lds_spheres_tab != kNone ? lds_row<SphereGeom>(sc.lds_spheres_tab, idx) : const_row(sc.spheres, idx);
        return sphere_test(r.o - mk(g.cx, g.cy, g.cz), r.d, a, g.r2, tmin, tmax, t);
    }
    case REF_MSPHERE: {
        MSphereGeom g = const_row(sc.mspheres, idx);
        return sphere_test(r.o - msphere_center(g, r.tm, (sc.flags & SCENE_MS_UNIT_TIME) != 0), r.d, a, g.r2, tmin, tmax, t);
    }
    default: {
        return quad_test_at(sc, idx, r, tmin, tmax, t);
    }
    }
}

#ifndef RT_PHASES
#define RT_PHASES 0  // diagnostic build: per-phase wave cycles and lane occupancy, summed into ray_counter[7] and [32..119]
#endif
#if RT_PHASES && RT_LANE_UNIT
#undef RT_PHASES
#define RT_PHASES 0  // the phases are render_kernel's: the feature and query units of a diagnostic build are the ordinary ones
#endif
#if RT_PHASES
#define PH_BEGIN() const unsigned long long ph_t0 = __builtin_readcyclecounter()
#define PH_END(k, cond)                                                   \
    do {                                                                  \
        ph.t[k] += __builtin_readcyclecounter() - ph_t0;                  \
        ph.l[k] += (unsigned long long)__popcll(__ballot(cond));          \
        ph.n[k] += 1ull;                                                  \
    } while (0)
struct PhaseSums {
    // 0 node, 1 leaf, 2 shade, 3 refill; per-lane shares inside divergent code (scaled x1024): 4 group/instance, 5 medium,
    // 6 primitive, 8 record+xforms, 9 box, 10 sub-BVH, 11 other geometry; wave level again: 16 box pass, 17 medium pass,
    // 18 object pass, 19 primitive pass (kind-batched kernels), 20 hit record, 21 scatter, 22 next camera ray, 23 pixel done
    unsigned long long t[24], l[24], n[24];
};
#define PH_ARG , PhaseSums &ph
#define PH_PASS , ph
#define PH_SUB_BEGIN() const unsigned long long ph_s0 = __builtin_readcyclecounter()
// per-lane event counts (summed over the wave at the end like the per-lane time shares): slot 14 = node visits
#define PH_COUNT(k) do { ph.l[k] += 1024ull; ph.n[k] += 1024ull; } while (0)
// inside divergent control flow the sums are per lane: each lane books its share (x1024), the wave adds them up at the end
#define PH_SUB_END(k)                                                                              \
    do {                                                                                           \
        const unsigned long long ph_pc = (unsigned long long)__popcll(__ballot(true));             \
        ph.t[k] += (__builtin_readcyclecounter() - ph_s0) * 1024ull / ph_pc;                       \
        ph.l[k] += 1024ull;                                                                        \
        ph.n[k] += 1024ull / ph_pc;                                                                \
    } while (0)
#else
#define PH_BEGIN() do { } while (0)
#define PH_END(k, cond) do { } while (0)
#define PH_ARG
#define PH_PASS
#define PH_SUB_BEGIN() do { } while (0)
#endif
#if RT_PHASES
// Survivor counts of the sphere-list scan through the filter, one pixel-parallel pass (wave-uniform: every active lane holds the same
// values).  The render loop adds them to the wave-level phase slots 12, 13 and 15 (device_scene.cpp prints them as the survivor table).
struct ScanSums {
    uint32_t groups, taken, spheres, appends, behind;  // groups of 4 examined / taken; spheres with a passing lane; lane appends; lanes behind
    uint32_t drains, drain_iters, drain_cycles;        // drain calls; wave max of count per call, summed; cycles spent draining
    uint32_t win_runs, win_trips, win_ranges, win_cycles;  // windowed runs scanned; trips and ranges of trips run in them; cycles of forming the windows
    uint32_t win_lane_trips;  // trips of those runs that each live lane's OWN extent needs, summed over the lanes (what a work-item form would run)
};
#define SS_ARG , ScanSums &ss
#define SS_PASS , ss
// The same for one pass of the grouped scan (scan_grouped; wave-uniform as well).  The render loop adds them to the wave-level phase
// slots 16, 17 and 18, which no sphere-list kernel uses otherwise (device_scene.cpp prints them as the grouped table).
struct GroupedSums {
    uint32_t rays, tests, survivors, lane_max;  // L; exact-test blocks the wave executed; lanes that went on to the exact test; largest count of one lane
    uint32_t drains, filter_cycles, test_cycles;  // drain calls; cycles in the filter's part and in the exact tests' part of the pass
    // The packed fp32 branch queues its survivors (r36): there `tests` counts drain iterations (the wave's largest queue per drain,
    // summed), `survivors` appends, `test_cycles` the drains' cycles and `filter_cycles` the rest of the loop.
};
#define GS_ARG , GroupedSums &gs
#define GS_PASS , gs
#else
#define SS_ARG
#define SS_PASS
#define GS_ARG
#define GS_PASS
#define PH_COUNT(k) do { } while (0)
#define PH_SUB_END(k) do { } while (0)
#endif
// A general affine step (include/rtow.h rt_transform; flat_scene.h XF_AFFINE has the rows): x_world = L x_obj + t.  Only scenes that
// hold one (SCENE_AFFINE) are served by the units compiled with RT_AFFINE (kAffineUnit); every other unit compiles the two-way branch of
// Translate / RotateY alone, the code it compiled before there was a third kind.
// affine_rows: M p for the matrix whose rows are xforms[row .. row + 2], each row ((m0 * p.x) + (m1 * p.y)) + (m2 * p.z).
DEV Vec affine_rows(const DeviceScene &sc, uint32_t row, Vec p)
{
    const Xform r0 = get_xform(sc, row), r1 = get_xform(sc, row + 1), r2 = get_xform(sc, row + 2);
    return mk(((r0.a * p.x) + (r0.b * p.y)) + (r0.c * p.z), ((r1.a * p.x) + (r1.b * p.y)) + (r1.c * p.z), ((r2.a * p.x) + (r2.b * p.y)) + (r2.c * p.z));
}
// head: the step's first row (x, holding t).  o' = Li (o - t), d' = Li d; the time stays and d' is not normalised, so the child's t is the world's.
DEV void affine_to_local(const DeviceScene &sc, uint32_t head, const Xform &x, Ray &lr)
{
    lr.o = affine_rows(sc, head + 4, lr.o - mk(x.a, x.b, x.c));
    lr.d = affine_rows(sc, head + 4, lr.d);
}
// The way back of the hit record: P = (L P') + t; n = Li^T n', renormalised at every such step.
DEV void affine_to_world(const DeviceScene &sc, uint32_t head, Vec &p, Vec &n)
{
    const Xform t = get_xform(sc, head);
    p = affine_rows(sc, head + 1, p) + mk(t.a, t.b, t.c);
    const Xform i0 = get_xform(sc, head + 4), i1 = get_xform(sc, head + 5), i2 = get_xform(sc, head + 6);
    const Vec m = mk(((i0.a * n.x) + (i1.a * n.y)) + (i2.a * n.z), ((i0.b * n.x) + (i1.b * n.y)) + (i2.b * n.z), ((i0.c * n.x) + (i1.c * n.y)) + (i2.c * n.z));
    n = (1.0 / sqrt(length_sq(m))) * m;
}
// A moving affine step (include/rtow.h rt_moving_transform; flat_scene.h XF_MOVING has the rows): the step above with its matrix keyed at
// two times.  Per ray: s = clamp((tm - time0) / dtime, 0, 1) (a NaN time sees key 0: fmax drops it), L = L0 + (s * dL), t = t0 + (s * dt)
// entry by entry, Li from L by rt_transform's cofactor formula.  Nothing of it is kept between the walks: make_surface forms the same
// L and Li again from the same tm, so the way back uses the bits the way in used, and no walk carries eighteen doubles for the rest of
// a bounce.  Li's rows are M.i[0..2], L's M.l[0..2].
// Only the second pass of an affine unit (kMovingUnit) compiles the step into its walks, as their unlikely branch: a scene whose chains
// hold static steps alone runs the walks without it.  moving_local / moving_world read the step's rows through a generic pointer,
// from LDS or from global memory as the table is staged.
struct MovingPose { Vec l[3], i[3], t; };
struct VecPair { Vec a, b; };
DEV MovingPose moving_pose(const Xform *rows, double tm)
{
    const Xform t0 = rows[0], dt = rows[4], key = rows[8];
    double s = (tm - key.a) / key.b;
    s = fmin(fmax(s, 0.0), 1.0);
    MovingPose m;
    for (uint32_t r = 0; r < 3; r++) {
        const Xform a = rows[1 + r], d = rows[5 + r];
        m.l[r] = mk(a.a + (s * d.a), a.b + (s * d.b), a.c + (s * d.c));
    }
    m.t = mk(t0.a + (s * dt.a), t0.b + (s * dt.b), t0.c + (s * dt.c));
    const Vec l0 = m.l[0], l1 = m.l[1], l2 = m.l[2];
    const double c00 = (l1.y * l2.z) - (l1.z * l2.y), c01 = (l1.z * l2.x) - (l1.x * l2.z), c02 = (l1.x * l2.y) - (l1.y * l2.x);
    const double c10 = (l0.z * l2.y) - (l0.y * l2.z), c11 = (l0.x * l2.z) - (l0.z * l2.x), c12 = (l0.y * l2.x) - (l0.x * l2.y);
    const double c20 = (l0.y * l1.z) - (l0.z * l1.y), c21 = (l0.z * l1.x) - (l0.x * l1.z), c22 = (l0.x * l1.y) - (l0.y * l1.x);
    const double det = ((l0.x * c00) + (l0.y * c01)) + (l0.z * c02);
    m.i[0] = mk(c00 / det, c10 / det, c20 / det);
    m.i[1] = mk(c01 / det, c11 / det, c21 / det);
    m.i[2] = mk(c02 / det, c12 / det, c22 / det);
    return m;
}
DEV Vec pose_rows(const Vec (&m)[3], Vec p)
{
    return mk(((m[0].x * p.x) + (m[0].y * p.y)) + (m[0].z * p.z), ((m[1].x * p.x) + (m[1].y * p.y)) + (m[1].z * p.z), ((m[2].x * p.x) + (m[2].y * p.y)) + (m[2].z * p.z));
}
// rows: the step's kMovingRows rows.  o' = Li (o - t), d' = Li d with this ray's matrices.
DEV VecPair moving_local(const Xform *rows, double tm, Vec o, Vec d)
{
    const MovingPose m = moving_pose(rows, tm);
    return VecPair{pose_rows(m.i, o - m.t), pose_rows(m.i, d)};
}
// P = (L P') + t; n = Li^T n', renormalised.
DEV VecPair moving_world(const Xform *rows, double tm, Vec p, Vec n)
{
    const MovingPose m = moving_pose(rows, tm);
    const Vec v = mk(((m.i[0].x * n.x) + (m.i[1].x * n.y)) + (m.i[2].x * n.z), ((m.i[0].y * n.x) + (m.i[1].y * n.y)) + (m.i[2].y * n.z), ((m.i[0].z * n.x) + (m.i[1].z * n.y)) + (m.i[2].z * n.z));
    return VecPair{pose_rows(m.l, p) + m.t, (1.0 / sqrt(length_sq(v))) * v};
}
DEV const Xform *xform_rows(const DeviceScene &sc, uint32_t i)
{
    return (sc.lds_xforms != kNone ? reinterpret_cast<const Xform *>(lds_raw + sc.lds_xforms) : sc.xforms) + i;
}
DEV void moving_to_local(const DeviceScene &sc, uint32_t head, Ray &lr)
{
    const VecPair v = moving_local(xform_rows(sc, head), lr.tm, lr.o, lr.d);
    lr.o = v.a;
    lr.d = v.b;
}
DEV void moving_to_world(const DeviceScene &sc, uint32_t head, double tm, Vec &p, Vec &n)
{
    const VecPair v = moving_world(xform_rows(sc, head), tm, p, n);
    p = v.a;
    n = v.b;
}
// Ray into the object space of a composite leaf: Translate (R/Instance.h:46) and RotateY (:121-131)
// applied outermost first.
DEV Ray to_object_space(const DeviceScene &sc, const ObjectRec &o, const Ray &r)
{
    Ray lr = r;
    for (uint32_t k = 0; k < o.xf_count; k++) {
        Xform x = get_xform(sc, o.xf_first + k);
        if (x.kind == XF_TRANSLATE) {
            lr.o = lr.o - mk(x.a, x.b, x.c);
        } else if (!kAffineUnit || x.kind == XF_ROTATE_Y) {
            double st = x.a, ct = x.b;
            lr.o = mk((ct * lr.o.x) - (st * lr.o.z), lr.o.y, (st * lr.o.x) + (ct * lr.o.z));
            lr.d = mk((ct * lr.d.x) - (st * lr.d.z), lr.d.y, (st * lr.d.x) + (ct * lr.d.z));
        } else if (!kMovingUnit || __builtin_expect(x.kind == XF_AFFINE, 1)) {
            affine_to_local(sc, o.xf_first + k, x, lr);
            k += kAffineRows - 1;
        } else {
            moving_to_local(sc, o.xf_first + k, lr);
            k += kMovingRows - 1;
        }
    }
    return lr;
}

DEV bool box_test(double xlo, double xhi, double ylo, double yhi, double zlo, double zhi, const Ray &r, Vec inv,
                  double tmin, double tmax);

// Sub-BVH over a large group's primitives (threaded like the world BVH; nodes stay in global memory / L2).
DEV bool subbvh_closest(const DeviceScene &sc, uint32_t root, const Ray &lr, double a, double tmin, double tmax,
                        double &t_best, uint32_t &ref_best)
{
    Vec inv = mk(1.0 / lr.d.x, 1.0 / lr.d.y, 1.0 / lr.d.z);
    double closest = tmax;
    bool any = false;
    uint32_t n = root;
    while (n != kNone) {
        BvhNodeRec node = sc.nodes[n];
        uint32_t next = node.escape;
        if (box_test(node.xlo, node.xhi, node.ylo, node.yhi, node.zlo, node.zhi, lr, inv, tmin, closest)) {
            if ((node.a >> kRefShift) == REF_INNER) {
                next = n + 1;
            } else {
                double t;
                if (prim_test(sc, node.a, lr, a, tmin, closest, t)) {
                    any = true;
                    closest = t;
                    ref_best = node.a;
                }
                if (node.b != node.a && prim_test(sc, node.b, lr, a, tmin, closest, t)) {
                    any = true;
                    closest = t;
                    ref_best = node.b;
                }
            }
        }
        n = next;
    }
    t_best = closest;
    return any;
}

// Closest hit over a composite leaf's geometry (R/HittableList.h:39-57 for groups).
DEV bool geom_closest(const DeviceScene &sc, const ObjectRec &o, const Ray &lr, double tmin, double tmax,
                      double &t_best, uint32_t &ref_best)
{
    double a = dot(lr.d, lr.d);
    bool any = false;
    double closest = tmax;
    if (o.geom_kind == GEOM_BVH) return subbvh_closest(sc, o.first, lr, a, tmin, tmax, t_best, ref_best);
    switch (o.geom_kind) {
    case GEOM_SINGLE: {
        double t;
        if (prim_test(sc, o.first, lr, a, tmin, closest, t)) {
            any = true;
            closest = t;
            ref_best = o.first;
        }
        break;
    }
    case GEOM_SPHERES:
        for (uint32_t k = 0; k < o.count; k++) {
            SphereGeom g = get_sphere(sc, o.first + k);
            double t;
            if (sphere_test(lr.o - mk(g.cx, g.cy, g.cz), lr.d, a, g.r2, tmin, closest, t)) {
                any = true;
                closest = t;
                ref_best = make_ref(REF_SPHERE, o.first + k);
            }
        }
        break;
    case GEOM_MSPHERES:
        for (uint32_t k = 0; k < o.count; k++) {
            MSphereGeom g = sc.mspheres[o.first + k];
            double t;
            if (sphere_test(lr.o - msphere_center(g, lr.tm), lr.d, a, g.r2, tmin, closest, t)) {
                any = true;
                closest = t;
                ref_best = make_ref(REF_MSPHERE, o.first + k);
            }
        }
        break;
    case GEOM_BOX:
        any = box_closest(sc, get_box(sc, o.first), lr, tmin, tmax, closest, ref_best);
        break;
    case GEOM_QUADS:
        for (uint32_t k = 0; k < o.count; k++) {
            double t;
            if (quad_test_at(sc, o.first + k, lr, tmin, closest, t)) {
                any = true;
                closest = t;
                ref_best = make_ref(REF_QUAD, o.first + k);
            }
        }
        break;
    default:
        for (uint32_t k = 0; k < o.count; k++) {
            uint32_t ref = sc.items[o.first + k];
            double t;
            if (prim_test(sc, ref, lr, a, tmin, closest, t)) {
                any = true;
                closest = t;
                ref_best = ref;
            }
        }
        break;
    }
    t_best = closest;
    return any;
}

// Composite leaf: instance chain and, for media, the stochastic volume hit (R/ConstantMedium.h:52-94).
// MED: what the caller knows about the leaf -- 1 a ConstantMedium, 0 not one, -1 look at the object record.
// object_span: the geometric part -- the instance chain, then one closest-hit query over [tmin, tmax] for a surface (t1, pref)
// or, for a medium, the two boundary queries of R/ConstantMedium.h:58-64 (t1, t2, unclipped).  false: nothing hit.
template <class T, int MED>
DEV bool object_span(const DeviceScene &sc, uint32_t oi, const Ray &r, double tmin, double tmax, bool &medium, MediumRec &med, uint32_t &medium_index,
                     double &t1, double &t2, uint32_t &pref PH_ARG)
{
#if RT_PHASES
    const unsigned long long ph_o0 = __builtin_readcyclecounter();
#endif
    ObjectRec o = get_object(sc, oi);
    Ray lr = to_object_space(sc, o, r);
#if RT_PHASES
    {
        // force the loads to land before the stamp
        asm volatile("" ::"v"(lr.o.x), "v"(lr.d.z), "v"(o.first));
        const unsigned long long ph_s0 = ph_o0;
        PH_SUB_END(8);
    }
#endif
    // surfaces: one closest-hit query over [tmin, tmax]; media: two boundary queries (R/ConstantMedium.h:58-64)
    medium = T::MEDIA && (MED < 0 ? o.medium != kNone : MED == 1);
    medium_index = o.medium;
    t1 = 0.0;
    t2 = 0.0;
    pref = kNone;
    if (medium) med = get_medium(sc, o.medium);
    if (medium && o.geom_kind == GEOM_SINGLE && (o.first >> kRefShift) == REF_SPHERE) {
        // The usual boundary: one sphere.  Both queries of R/ConstantMedium.h:58-64 share oc, b, c and the
        // discriminant (R/Sphere.h:28-34); only the root selection (:36-60) runs twice.  A sphere without transforms
        // has its row repeated in the medium record (one table less to chase through).
        SphereGeom g;
        if (med.sphere != kNone) g = SphereGeom{med.cx, med.cy, med.cz, med.r2};
        else g = get_sphere(sc, o.first & kRefIndexMask);
        const Vec oc = lr.o - mk(g.cx, g.cy, g.cz);
        const double a = dot(lr.d, lr.d);
        const double b = dot(oc, lr.d);
        const double c = dot(oc, oc) - g.r2;
        const double disc = b * b - a * c;
        if (!(disc > 0.0)) return false;
        if (!sphere_roots(b, disc, a, -DBL_MAX, DBL_MAX, t1)) return false;
        if (!sphere_roots(b, disc, a, t1 + 0.0001, DBL_MAX, t2)) return false;
    } else {
        for (int pass = 0; pass < 2; pass++) {  // one inlined copy of the geometry query
            const double lo = medium ? (pass == 0 ? -DBL_MAX : t1 + 0.0001) : tmin;
            const double hi = medium ? DBL_MAX : tmax;
            double t;
            PH_SUB_BEGIN();
            const bool got = geom_closest(sc, o, lr, lo, hi, t, pref);
#if RT_PHASES
            asm volatile("" ::"v"(t));
#endif
            PH_SUB_END(o.geom_kind == GEOM_BOX ? 9 : (o.geom_kind == GEOM_BVH ? 10 : 11));
            if (!got) return false;
            if (pass == 0) t1 = t;
            else t2 = t;
            if (!medium) break;
        }
    }
    return true;
}

// The rest of ConstantMedium::Hit (R/ConstantMedium.h:66-93) given its two boundary hits: clip to [tmin, tmax], draw, compare.
DEV bool medium_draw(double neg_inv_density, uint32_t medium_index, uint32_t oi, const Ray &r, double tmin, double tmax, double t1, double t2,
                     HitInfo &best, Xorwow &rng)
{
    if (t1 < tmin) t1 = tmin;
    if (t2 > tmax) t2 = tmax;
    if (t1 >= t2) return false;
    if (t1 < 0.0) t1 = 0.0;
    double ray_len = length(r.d);
    double inside = (t2 - t1) * ray_len;
    // log(curand_uniform(..)) has a float argument: the float overload is selected on the reference's
    // toolchain; evaluated here as the correctly rounded fp32 log.
    float lg = (float)log((double)xorwow_uniform(rng));
    double hit_dist = neg_inv_density * (double)lg;
    if (hit_dist > inside) return false;
    best.t = t1 + hit_dist / ray_len;
    best.ref = make_ref(REF_MEDIUM, medium_index);
    best.obj = oi;
    return true;
}

template <class T, int MED = -1>
DEV bool object_test(const DeviceScene &sc, uint32_t oi, const Ray &r, double tmin, double tmax, HitInfo &best, Xorwow &rng PH_ARG)
{
    bool medium;
    MediumRec med{};
    uint32_t medium_index, pref;
    double t1, t2;
    if (!object_span<T, MED>(sc, oi, r, tmin, tmax, medium, med, medium_index, t1, t2, pref PH_PASS)) return false;
    if (!medium) {
        best.t = t1;
        best.ref = pref;
        best.obj = oi;
        return true;
    }
    return medium_draw(med.neg_inv_density, medium_index, oi, r, tmin, tmax, t1, t2, best, rng);
}

// ------------------------------------------------------------------------------------------------
// General nesting: a composite kept as the reference's own object tree (flat_scene.h TreeNodeRec), evaluated by making
// the reference's calls in the reference's order with an explicit stack -- Translate::Hit / RotateY::Hit
// (R/Instance.h:41-56,116-150), HittableList::Hit (R/HittableList.h:39-57), ConstantMedium::Hit (R/ConstantMedium.h:52-94:
// two boundary calls, one draw) and BvhNode::Hit (R/BvhNode.h:101-158, incl. BvhNode objects among the leaves, which its
// loop walks as inner nodes).  The hit record is the kernel's usual (t, primitive, where): the point, normal and their
// way back through the transforms are built once per bounce by make_surface from the winning node's chain.  A failed
// call never touches the record (as in the reference, where every Hit writes only on success); a medium, whose boundary
// calls write a record of their own, keeps the caller's in its frame.
// ------------------------------------------------------------------------------------------------
struct TreeFrame {
    uint32_t node;
    uint32_t step;     // LIST: next child; MEDIUM / transforms: 0, 1, 2; BVH: 0 visit, 1 after leaf a, 2 after leaf b
    uint32_t cursor;   // BVH: threaded node
    uint32_t any;
    double tmin, tmax; // the interval this call was made with
    double closest;    // LIST / BVH: closestSoFar;  MEDIUM: t of the first boundary hit
    HitInfo saved;     // MEDIUM: the caller's record
};

DEV Ray chain_ray(const DeviceScene &sc, uint32_t first, uint32_t count, const Ray &r)
{
    Ray lr = r;
    for (uint32_t k = 0; k < count; k++) {
        Xform x = get_xform(sc, first + k);
        if (x.kind == XF_TRANSLATE) {
            lr.o = lr.o - mk(x.a, x.b, x.c);
        } else if (!kAffineUnit || x.kind == XF_ROTATE_Y) {
            double st = x.a, ct = x.b;
            lr.o = mk((ct * lr.o.x) - (st * lr.o.z), lr.o.y, (st * lr.o.x) + (ct * lr.o.z));
            lr.d = mk((ct * lr.d.x) - (st * lr.d.z), lr.d.y, (st * lr.d.x) + (ct * lr.d.z));
        } else if (!kMovingUnit || __builtin_expect(x.kind == XF_AFFINE, 1)) {
            affine_to_local(sc, first + k, x, lr);
            k += kAffineRows - 1;
        } else {
            moving_to_local(sc, first + k, lr);
            k += kMovingRows - 1;
        }
    }
    return lr;
}

template <class T>
DEV bool tree_hit(const DeviceScene &sc, uint32_t root, const Ray &r, double tmin0, double tmax0, HitInfo &best, Xorwow &rng)
{
    TreeFrame stack[kTreeMaxDepth];
    int sp = 0;
    stack[0] = TreeFrame{root, 0u, kNone, 0u, tmin0, tmax0, tmax0, HitInfo{0.0, kNone, kNone}};
    bool ret = false;            // what the call that has just returned answered
    uint32_t chain_first = kNone, chain_count = 0;  // the chain `lr` was computed for
    Ray lr = r;
    for (;;) {
        TreeFrame &f = stack[sp];
        const TreeNodeRec n = sc.tree_nodes[f.node];
        if (n.chain_first != chain_first || n.chain_count != chain_count) {  // always from the world ray: same bits every time
            lr = chain_ray(sc, n.chain_first, n.chain_count, r);
            chain_first = n.chain_first;
            chain_count = n.chain_count;
        }
        uint32_t call = kNone;   // child to call next, with [call_tmin, call_tmax]
        double call_tmin = 0.0, call_tmax = 0.0;
        bool answer = false;  // what this call answers, unless it first calls a child (`call`)
        switch (n.kind) {
        case TN_PRIM: {
            double t;
            answer = prim_test(sc, n.a, lr, dot(lr.d, lr.d), f.tmin, f.tmax, t);
            if (answer) {
                best.t = t;
                best.ref = n.a;
                best.obj = kTreeObjBit | f.node;
            }
            break;
        }
        case TN_TRANSLATE:
        case TN_ROTATE_Y:
#if RT_AFFINE
        case TN_TRANSFORM:
#endif
            if (f.step == 0) {
                f.step = 1;
                call = n.a; call_tmin = f.tmin; call_tmax = f.tmax;
            } else {
                answer = ret;
            }
            break;
        case TN_LIST:
            if (f.step > 0 && ret) {
                f.any = 1;
                f.closest = best.t;
            }
            if (f.step < n.b) {
                call = sc.tree_items[n.a + f.step];
                call_tmin = f.tmin; call_tmax = f.closest;
                f.step++;
            } else {
                answer = f.any != 0;
            }
            break;
        case TN_MEDIUM: {
            if (f.step == 0) {
                f.saved = best;
                f.step = 1;
                call = n.a; call_tmin = -DBL_MAX; call_tmax = DBL_MAX;
            } else if (f.step == 1) {
                if (!ret) {
                    best = f.saved;
                } else {
                    f.closest = best.t;  // rec1.T
                    f.step = 2;
                    call = n.a; call_tmin = f.closest + 0.0001; call_tmax = DBL_MAX;
                }
            } else {
                double t1 = f.closest, t2 = best.t;
                const bool second = ret;
                best = f.saved;
                if (second) {
                    if (t1 < f.tmin) t1 = f.tmin;
                    if (t2 > f.tmax) t2 = f.tmax;
                    if (t1 < t2) {
                        if (t1 < 0.0) t1 = 0.0;
                        const MediumRec med = get_medium(sc, n.b);
                        const double ray_len = length(lr.d);
                        const double inside = (t2 - t1) * ray_len;
                        const float lg = (float)log((double)xorwow_uniform(rng));  // see object_test
                        const double hit_dist = med.neg_inv_density * (double)lg;
                        if (!(hit_dist > inside)) {
                            best.t = t1 + hit_dist / ray_len;
                            best.ref = make_ref(REF_MEDIUM, n.b);
                            best.obj = kTreeObjBit | f.node;
                            answer = true;
                        }
                    }
                }
            }
            break;
        }
        default: {  // TN_BVH
            if (f.cursor == kNone) f.cursor = n.a;  // first entry: the root of this BvhNode's threaded nodes
            for (;;) {
                const BvhNodeRec node = sc.tree_bvh[f.cursor];
                if (f.step == 0) {
                    const Vec inv = mk(1.0 / lr.d.x, 1.0 / lr.d.y, 1.0 / lr.d.z);
                    if (!box_test(node.xlo, node.xhi, node.ylo, node.yhi, node.zlo, node.zhi, lr, inv, f.tmin, f.closest)) {
                        if (node.escape == kNone) {
                            answer = f.any != 0;
                            break;
                        }
                        f.cursor = node.escape;
                        continue;
                    }
                    f.step = 1;
                    if ((node.a >> kRefShift) != REF_INNER) {
                        call = node.a & kRefIndexMask; call_tmin = f.tmin; call_tmax = f.closest;
                        break;
                    }
                    ret = false;
                }
                if (f.step == 1) {
                    if ((node.a >> kRefShift) != REF_INNER && ret) {
                        f.any = 1;
                        f.closest = best.t;
                    }
                    f.step = 2;
                    if ((node.b >> kRefShift) != REF_INNER) {
                        call = node.b & kRefIndexMask; call_tmin = f.tmin; call_tmax = f.closest;
                        break;
                    }
                    ret = false;
                }
                // step 2: both children have been dealt with
                if ((node.b >> kRefShift) != REF_INNER && ret) {
                    f.any = 1;
                    f.closest = best.t;
                }
                f.step = 0;
                const bool has_inner = (node.a >> kRefShift) == REF_INNER || (node.b >> kRefShift) == REF_INNER;
                const uint32_t next = has_inner ? f.cursor + 1u : node.escape;
                if (next == kNone) {
                    answer = f.any != 0;
                    break;
                }
                f.cursor = next;
            }
            break;
        }
        }
        if (call != kNone) {
            if (sp + 1 >= (int)kTreeMaxDepth) return false;  // cannot happen: rt_scene_commit refuses deeper trees
            sp++;
            stack[sp] = TreeFrame{call, 0u, kNone, 0u, call_tmin, call_tmax, call_tmax, HitInfo{0.0, kNone, kNone}};
            ret = false;
            continue;
        }
        // done: return `answer` to the caller
        ret = answer;
        if (sp == 0) return ret;
        sp--;
    }
}

// a leaf whose test may draw random numbers (tagged by the flattener): a ConstantMedium object, or a tree (may hold media)
DEV bool is_medium_leaf(uint32_t ref) { return (ref >> kRefShift) == REF_MOBJECT || (ref >> kRefShift) == REF_TREE; }

template <class T>
DEV bool leaf_test(const DeviceScene &sc, uint32_t ref, const Ray &r, double a, double tmin, double tmax, HitInfo &best, Xorwow &rng PH_ARG)
{
    if constexpr (T::COMPOSITE) {
        if ((ref >> kRefShift) == REF_BOX) {
            PH_SUB_BEGIN();
            double t;
            uint32_t face = kNone;
            const bool found = box_closest(sc, get_box(sc, ref & kRefIndexMask), r, tmin, tmax, t, face);
            if (found) {
                best.t = t;
                best.ref = face;
                best.obj = kNone;
            }
            PH_SUB_END(9);
            return found;
        }
        if ((ref >> kRefShift) == REF_OBJECT || (ref >> kRefShift) == REF_MOBJECT) {
            PH_SUB_BEGIN();
            const bool found = object_test<T>(sc, ref & kRefIndexMask, r, tmin, tmax, best, rng PH_PASS);
            PH_SUB_END(is_medium_leaf(ref) ? 5 : 4);
            return found;
        }
    }
    if constexpr (T::NESTED) {
        if ((ref >> kRefShift) == REF_TREE) return tree_hit<T>(sc, ref & kRefIndexMask, r, tmin, tmax, best, rng);
    }
    PH_SUB_BEGIN();
    double t;
    const bool found = prim_test(sc, ref, r, a, tmin, tmax, t);
    if (found) {
        best.t = t;
        best.ref = ref;
        best.obj = kNone;
    }
    PH_SUB_END(6);
    return found;
}


// ------------------------------------------------------------------------------------------------
// world traversal
// ------------------------------------------------------------------------------------------------
// Slab test, R/AABB.h:68-98, with 1/d hoisted out of the node loop (same value every time).
DEV bool box_test(double xlo, double xhi, double ylo, double yhi, double zlo, double zhi, const Ray &r, Vec inv,
                  double tmin, double tmax)
{
    double t0 = (xlo - r.o.x) * inv.x, t1 = (xhi - r.o.x) * inv.x;
    tmin = fmax(tmin, fmin(t0, t1));
    tmax = fmin(tmax, fmax(t0, t1));
    t0 = (ylo - r.o.y) * inv.y;
    t1 = (yhi - r.o.y) * inv.y;
    tmin = fmax(tmin, fmin(t0, t1));
    tmax = fmin(tmax, fmax(t0, t1));
    t0 = (zlo - r.o.z) * inv.z;
    t1 = (zhi - r.o.z) * inv.z;
    tmin = fmax(tmin, fmin(t0, t1));
    tmax = fmin(tmax, fmax(t0, t1));
    return tmax > tmin;
}

// Stackless walk in the reference's visiting order (R/BvhNode.h:101-158): a node's leaf children are
// tested where the node is visited; "pop" is the escape link.  The walk is resumable: a lane keeps its
// position (node index, closest hit so far) in registers, so that the kernel can interleave traversal
// bursts with shading and never makes 63 lanes wait for the one ray that visits 150 nodes.
constexpr uint32_t kWalkParked = 0x80000000u;
DEV bool walk_moving(uint32_t state) { return (int32_t)state >= 0; }
DEV bool walk_parked(uint32_t state) { return (int32_t)state < -1; }

struct Walk {
    Vec inv;          // 1 / direction (R/AABB.h:77,84,91 recompute it per node; same value)
    double a;         // dot(d, d)
    double closest;
    // Where the lane stands, in one word so that each of the wave's three questions is a single compare:
    //   moving  (state >= 0 as int32): `state` is the next node to visit;
    //   parked  (bit 31 set, not kNone): standing on bottom node `state & 0x7FFFFFFF` whose box was hit -- its leaves
    //           are tested in the next leaf phase;
    //   done    (kNone): the walk is complete (or no walk is in progress).
    uint32_t state;
    uint32_t oct_off;  // library-tree kernels: byte offset, inside a FastNodeF row, of the link pair of this ray's direction octant
    // library-tree kernels: the ray as the fp32 slab test of their node boxes wants it (box_test_f): 1 / direction and the
    // origin, in fp32 (`inv` above is then unused: those boxes are never tested in fp64)
    float ivx, ivy, ivz, cx, cy, cz;  // 1 / direction; origin
    bool any;
};

template <bool LIBRARY_TREE = false>
DEV void walk_begin(Walk &w, const Ray &r, double tmax)
{
    w.oct_off = 32u + 4u * ((r.d.x < 0.0 ? 1u : 0u) | (r.d.y < 0.0 ? 2u : 0u) | (r.d.z < 0.0 ? 4u : 0u));
    if constexpr (LIBRARY_TREE) {
        w.ivx = 1.0f / (float)r.d.x; w.ivy = 1.0f / (float)r.d.y; w.ivz = 1.0f / (float)r.d.z;
        w.cx = (float)r.o.x; w.cy = (float)r.o.y; w.cz = (float)r.o.z;
    } else {
        w.inv = mk(1.0 / r.d.x, 1.0 / r.d.y, 1.0 / r.d.z);
    }
    w.a = dot(r.d, r.d);
    w.closest = tmax;
    w.state = 0;
    w.any = false;
}

DEV uint32_t leaf_kind(uint32_t ref);
constexpr uint32_t kWalkKindShift = 28;  // kind-batched kernels: bits 28-29 of a parked state = kind of the pending leaf

// One inner-node step: box test, then descend / escape; a bottom node whose box is hit parks the lane.
template <bool BATCH = false>
DEV void walk_node(const NodeView &nv, const Ray &r, double tmin, Walk &w)
{
    const uint32_t n = w.state;
    double xlo, xhi, ylo, yhi, zlo, zhi;
    uint32_t na, next;
    if (nv.in_lds) {
        xlo = lds_node_f64(nv.n, 0, n); xhi = lds_node_f64(nv.n, 1, n); ylo = lds_node_f64(nv.n, 2, n);
        yhi = lds_node_f64(nv.n, 3, n); zlo = lds_node_f64(nv.n, 4, n); zhi = lds_node_f64(nv.n, 5, n);
        na = lds_node_u32(nv.n, 0, n); next = lds_node_u32(nv.n, 2, n);
    } else {
        const BvhNodeRec *node = nv.global + n;
        xlo = node->xlo; xhi = node->xhi; ylo = node->ylo; yhi = node->yhi; zlo = node->zlo; zhi = node->zhi;
        na = node->a; next = node->escape;
    }
    // selects, not branches: hit an inner node -> its first child; hit a bottom node -> park on it until the leaf phase;
    // missed -> the escape link
    const bool hit = box_test(xlo, xhi, ylo, yhi, zlo, zhi, r, w.inv, tmin, w.closest);
    uint32_t park = n | kWalkParked;
    if constexpr (BATCH) park |= leaf_kind(na) << kWalkKindShift;  // the wave sorts its parked lanes by this, without a table read
    const uint32_t down = (na >> kRefShift) == REF_INNER ? n + 1u : park;
    w.state = hit ? down : next;
}

// Leaf phase for a parked lane: the bottom node's one or two leaves, in the reference's order.
template <class T>
DEV void walk_leaves(const DeviceScene &sc, const NodeView &nv, const Ray &r, double tmin, Walk &w, HitInfo &best, Xorwow &rng PH_ARG)
{
    const uint32_t n = w.state & ~kWalkParked;
    uint32_t na, nb, next;
    if (nv.in_lds) {
        na = lds_node_u32(nv.n, 0, n); nb = lds_node_u32(nv.n, 1, n); next = lds_node_u32(nv.n, 2, n);
    } else {
        const BvhNodeRec *node = nv.global + n;
        na = node->a; nb = node->b; next = node->escape;
    }
    // span-1 nodes hold the same leaf twice (R/BvhNode.h:63-67).  Re-testing a surface with
    // tmax = its own t changes nothing; a medium draws again, so only media are re-tested.
    bool again = nb != na;
    if constexpr (T::MEDIA) again = again || is_medium_leaf(nb);
    if constexpr (!T::COMPOSITE) {
        // The common bottom node of a sphere world: two moving-sphere rows (static spheres are stored as such rows too,
        // see unify_spheres).  Both rows are fetched together -- one round trip to L2 instead of two -- and tested in
        // the reference's order.
        if ((na >> kRefShift) == REF_MSPHERE && (nb >> kRefShift) == REF_MSPHERE) {
            const bool unit_time = (sc.flags & SCENE_MS_UNIT_TIME) != 0;
            const MSphereGeom ga = sc.mspheres[na & kRefIndexMask], gb = sc.mspheres[nb & kRefIndexMask];
            double t;
            if (sphere_test(r.o - msphere_center(ga, r.tm, unit_time), r.d, w.a, ga.r2, tmin, w.closest, t)) {
                w.any = true;
                w.closest = t;
                best.t = t;
                best.ref = na;
                best.obj = kNone;
            }
            if (again && sphere_test(r.o - msphere_center(gb, r.tm, unit_time), r.d, w.a, gb.r2, tmin, w.closest, t)) {
                w.any = true;
                w.closest = t;
                best.t = t;
                best.ref = nb;
                best.obj = kNone;
            }
            w.state = next;
            return;
        }
    }
    for (int c = 0; c < 2; c++) {  // one inlined copy of the leaf test
        if (c == 1 && !again) break;
        if (leaf_test<T>(sc, c ? nb : na, r, w.a, tmin, w.closest, best, rng PH_PASS)) {
            w.any = true;
            w.closest = best.t;
        }
    }
    w.state = next;
}

// ---- the library's own tree (FastNodeF): same resumable walk, 68-byte rows, links chosen by the ray's octant ----
constexpr uint32_t kFastNodeBytes = (uint32_t)sizeof(FastNodeF);
static_assert(sizeof(FastNodeF) == 68 && offsetof(FastNodeF, a) == 24 && offsetof(FastNodeF, link) == 32, "row layout: box 24, leaf refs 8, links 32, pad 4");
// Conservative slab test in fp32.  The boxes of the library's tree only prune: a ray that passes one it should not merely
// visits a node in vain, a ray that FAILS one it should pass would lose a hit.  So the test may err only towards "hit":
//   t = (lo - o) * (1/d) like R/AABB.h:77-97, in fp32.  Its error against the exact (lo - o) / d is at most
//   2^-22 (|lo| + |o|) / |d| (the fp32 copies of o and of 1/d, the subtraction, the product), and the rows are 2^-19 of the
//   scene's reach (>= |lo|, |o|) wider than the boxes (device_scene.cpp): several times that; the ray's interval
//   [tmin, closest] is a little wider too.
// A zero direction component gives infinities, and a NaN where the origin lies in the plane: v_min / v_max drop NaNs, an
// infinite bound never cuts the interval short on the wrong side -- the behaviour of R/AABB.h:68-98 in fp64.  (The cheaper
// lo * (1/d) - o * (1/d), one fma per plane, is NOT safe: with 1/d infinite both terms are, and inf - inf or -inf - inf
// discards or inverts the slab -- measured: 1.6 % of C5's pixels at 5000 spp, from directions with a component exactly 0.)
DEV bool box_test_f(float xlo, float xhi, float ylo, float yhi, float zlo, float zhi, const Walk &w, float tmin, double closest)
{
    const float t0x = (xlo - w.cx) * w.ivx, t1x = (xhi - w.cx) * w.ivx;
    const float t0y = (ylo - w.cy) * w.ivy, t1y = (yhi - w.cy) * w.ivy;
    const float t0z = (zlo - w.cz) * w.ivz, t1z = (zhi - w.cz) * w.ivz;
    const float cf = (float)closest * 1.000002f;  // >= closest (round to nearest loses at most 2^-24); +inf stays +inf
    const float tnear = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tmin));
    const float tfar = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), cf));
    return tfar > tnear;
}
DEV bool fast_row_hit(uint32_t base, const Walk &w, double closest)
{
    const RT_LDS float *b = (const RT_LDS float *)(lds_raw + base);
    return box_test_f(b[0], b[1], b[2], b[3], b[4], b[5], w, 0.000999f, closest);  // tmin = 0.001, a little early
}
// The rows are only ever read from LDS (the launcher falls back to the reference-tree kernel when they do not fit): a
// branch between an LDS and a global copy made the compiler merge the two into generic pointers and flat loads.
DEV void walk_node_fast(const Ray &r, double tmin, Walk &w)
{
    const uint32_t n = w.state;
    const uint32_t base = __umul24(n, kFastNodeBytes);
    const uint32_t links = *reinterpret_cast<const uint32_t *>(lds_raw + base + w.oct_off);
    const bool hit = fast_row_hit(base, w, w.closest);
    const uint32_t first = links & 0xFFFFu, esc = links >> 16;
    const uint32_t down = (first & kFastBottom) ? (n | kWalkParked) : first;  // a bottom node's hit link says "park here"
    const uint32_t next = esc == kFastEnd ? kNone : esc;
    w.state = hit ? down : next;
}
// The same for the segmented walk's usual case -- no limit on the leaf positions: the parked state carries the kind of the
// pending leaf (kind-batched leaf phases), which the bottom node's hit link holds in the place the state wants it.
static_assert(kFastBottom << 16 == kWalkParked && kWalkKindShift == 28, "hit link of a bottom node << 16 = parked bit | kind");
DEV void walk_node_open(const Ray &r, double tmin, Walk &w)
{
    const uint32_t n = w.state;
    const uint32_t base = __umul24(n, kFastNodeBytes);
    const uint32_t links = *reinterpret_cast<const uint32_t *>(lds_raw + base + w.oct_off);
    const bool hit = fast_row_hit(base, w, w.closest);
    const uint32_t first = links & 0xFFFFu, esc = links >> 16;
    const uint32_t down = (first & kFastBottom) ? (n | (first << 16)) : first;
    const uint32_t next = esc == kFastEnd ? kNone : esc;
    w.state = hit ? down : next;
}
DEV void walk_leaves_fast(const DeviceScene &sc, const Ray &r, double tmin, Walk &w, HitInfo &best)
{
    const uint32_t n = w.state & ~kWalkParked;
    const uint32_t base = __umul24(n, kFastNodeBytes);
    const uint32_t na = *reinterpret_cast<const uint32_t *>(lds_raw + base + 24u);
    const uint32_t nb = *reinterpret_cast<const uint32_t *>(lds_raw + base + 28u);
    const uint32_t links = *reinterpret_cast<const uint32_t *>(lds_raw + base + w.oct_off);
    const uint32_t esc = links >> 16;
    const uint32_t next = esc == kFastEnd ? kNone : esc;
    if ((na >> kRefShift) == REF_MSPHERE && nb != kNone && (nb >> kRefShift) == REF_MSPHERE) {  // both rows in one round trip
        const bool unit_time = (sc.flags & SCENE_MS_UNIT_TIME) != 0;
        const MSphereGeom ga = get_msphere(sc, na & kRefIndexMask), gb = get_msphere(sc, nb & kRefIndexMask);
        double t;
        if (sphere_test(r.o - msphere_center(ga, r.tm, unit_time), r.d, w.a, ga.r2, tmin, w.closest, t)) {
            w.any = true; w.closest = t; best.t = t; best.ref = na; best.obj = kNone;
        }
        if (sphere_test(r.o - msphere_center(gb, r.tm, unit_time), r.d, w.a, gb.r2, tmin, w.closest, t)) {
            w.any = true; w.closest = t; best.t = t; best.ref = nb; best.obj = kNone;
        }
        w.state = next;
        return;
    }
    if ((na >> kRefShift) == REF_MSPHERE && nb == kNone) {  // a bottom node of one sphere row
        const MSphereGeom ga = get_msphere(sc, na & kRefIndexMask);
        double t;
        if (sphere_test(r.o - msphere_center(ga, r.tm, (sc.flags & SCENE_MS_UNIT_TIME) != 0), r.d, w.a, ga.r2, tmin, w.closest, t)) {
            w.any = true; w.closest = t; best.t = t; best.ref = na; best.obj = kNone;
        }
        w.state = next;
        return;
    }
    for (int c = 0; c < 2; c++) {  // one inlined copy of the test
        const uint32_t ref = c ? nb : na;
        if (ref == kNone) break;
        double t;
        if (prim_test(sc, ref, r, w.a, tmin, w.closest, t)) {
            w.any = true; w.closest = t; best.t = t; best.ref = ref; best.obj = kNone;
        }
    }
    w.state = next;
}

// ---- segmented walk of a composite world (Traits::SEG) ----------------------------------------------------------------
// The same near-child-first walk over 88-byte rows, restricted to the leaves whose position in the reference's visiting
// order is below `hi` (the walk that leads up to a medium: what follows the medium in that order must not be seen yet):
// a node all of whose leaves come later counts as a box miss.  A bottom node parks the lane on its first leaf that is
// allowed (kWalkSecond set when that is leaf b).  Positions have no lower limit: a leaf met again by a later walk of the
// same ray answers as before or not at all (its test is repeated with the closest hit it helped to find).
DEV uint32_t leaf_kind(uint32_t ref);
constexpr uint32_t kWalkSecond = 0x40000000u;  // parked on the bottom node's SECOND leaf
DEV void walk_node_seg(const DeviceScene &sc, const Ray &r, double tmin, Walk &w, uint32_t hi)
{
    const uint32_t n = w.state;
    const uint32_t base = __umul24(n, kFastNodeBytes);
    const uint32_t na = *reinterpret_cast<const uint32_t *>(lds_raw + base + 24u);
    const uint32_t nb = *reinterpret_cast<const uint32_t *>(lds_raw + base + 28u);
    const uint32_t links = *reinterpret_cast<const uint32_t *>(lds_raw + base + w.oct_off);
    const uint32_t span = *reinterpret_cast<const uint32_t *>(lds_raw + sc.lds_fast_order + n * 8u);        // omin | omax << 16
    const uint32_t leaves = *reinterpret_cast<const uint32_t *>(lds_raw + sc.lds_fast_order + n * 8u + 4u);  // oa | ob << 16
    const bool inner = (na >> kRefShift) == REF_INNER;
    const uint32_t oa = leaves & 0xFFFFu, ob = leaves >> 16;
    const bool a_in = oa < hi, b_in = nb != kNone && ob < hi;
    const bool in_range = inner ? (span & 0xFFFFu) < hi : (a_in || b_in);
    const bool hit = in_range && fast_row_hit(base, w, w.closest);
    const uint32_t first = links & 0xFFFFu, esc = links >> 16;
    const uint32_t pending = a_in ? na : nb;
    const uint32_t park = n | kWalkParked | (a_in ? 0u : kWalkSecond) | (leaf_kind(pending) << kWalkKindShift);
    const uint32_t next = esc == kFastEnd ? kNone : esc;
    w.state = hit ? (inner ? first : park) : next;
}
// the pending leaf of a lane parked by walk_node_seg
DEV uint32_t seg_pending_leaf(uint32_t state)
{
    return *reinterpret_cast<const uint32_t *>(lds_raw + __umul24(state & 0x0FFFFFFFu, kFastNodeBytes) + ((state & kWalkSecond) ? 28u : 24u));
}
struct SegState {
    uint32_t lo, hi;  // the walk in progress (or just completed) covers the leaf positions [lo, hi); hi == kSegEnd: the ray's last walk
    uint32_t stage;   // next medium (index into seg_media) the ray has to deal with
};

// Composite worlds: the leaf phase runs one KIND of leaf at a time.  A box, a medium, an instance and a plain primitive
// are four different pieces of code; tested in one divergent pass the wave executes each of them with the few lanes
// that happen to stand on that kind (measured on the Book-2 final scene: 12-16 of 64 lanes per pass).  So a parked
// lane remembers which of its bottom node's two leaves is pending, the wave counts the pending leaves by kind, and a
// kind is run when enough lanes wait for it (or the walkers have run out, or this is the last round before the next
// look at the shading queue).  Each lane still meets its own leaves in the reference's order -- only when the wave
// executes them changes -- so the RNG draws of media are consumed exactly as before.
enum : uint32_t { LK_BOX = 0u, LK_MEDIUM = 1u, LK_OBJECT = 2u, LK_PRIM = 3u };
constexpr uint32_t kWalkNodeMask = 0x0FFFFFFFu;
DEV uint32_t leaf_kind(uint32_t ref)
{
    const uint32_t tag = ref >> kRefShift;
    return tag == REF_BOX ? LK_BOX : (tag == REF_MOBJECT ? LK_MEDIUM : (tag == REF_OBJECT ? LK_OBJECT : LK_PRIM));
}
// the pending leaf of a parked lane
DEV uint32_t walk_pending_leaf(const NodeView &nv, uint32_t state)
{
    const uint32_t n = state & kWalkNodeMask, word = (state & kWalkSecond) ? 1u : 0u;
    if (nv.in_lds) return lds_node_u32(nv.n, word, n);
    return word ? nv.global[n].b : nv.global[n].a;
}

template <class T, uint32_t K>
DEV bool leaf_test_kind(const DeviceScene &sc, uint32_t ref, const Ray &r, double a, double tmin, double tmax, HitInfo &best, Xorwow &rng PH_ARG)
{
    if constexpr (K == LK_BOX) {
        double t;
        uint32_t face = kNone;
        const bool found = box_closest(sc, get_box(sc, ref & kRefIndexMask), r, tmin, tmax, t, face);
        if (found) {
            best.t = t;
            best.ref = face;
            best.obj = kNone;
        }
        return found;
    } else if constexpr (K == LK_MEDIUM) {
        return object_test<T, 1>(sc, ref & kRefIndexMask, r, tmin, tmax, best, rng PH_PASS);
    } else if constexpr (K == LK_OBJECT) {
        return object_test<T, 0>(sc, ref & kRefIndexMask, r, tmin, tmax, best, rng PH_PASS);
    } else {
        double t;
        const bool found = prim_test(sc, ref, r, a, tmin, tmax, t);
        if (found) {
            best.t = t;
            best.ref = ref;
            best.obj = kNone;
        }
        return found;
    }
}

// One pass over the lanes whose pending leaf `ref` is of kind K: test it; if the node's other leaf is due (span-1 nodes
// hold the same leaf twice, R/BvhNode.h:63-67: only a medium is tested again, see walk_leaves) and is of the same kind
// it is tested in the same pass, otherwise the lane stays parked on it until that kind's pass.
template <class T, uint32_t K>
DEV void walk_leaf_pass(const DeviceScene &sc, const NodeView &nv, const Ray &r, double tmin, Walk &w, HitInfo &best, Xorwow &rng,
                        uint32_t ref PH_ARG, bool have_first = false, bool first_found = false, double first_t = 0.0,
                        uint32_t first_ref = kNone, uint32_t seg_lo = 0u, uint32_t seg_hi = 0u)
{
    const uint32_t n = w.state & kWalkNodeMask;
    uint32_t nb, next;
    [[maybe_unused]] bool b_in = false;  // segmented walk: the node's second leaf lies in the interval being walked
    if constexpr (T::SEG) {
        const uint32_t base = __umul24(n, kFastNodeBytes);
        nb = *reinterpret_cast<const uint32_t *>(lds_raw + base + 28u);
        const uint32_t esc = *reinterpret_cast<const uint32_t *>(lds_raw + base + w.oct_off) >> 16;
        next = esc == kFastEnd ? kNone : esc;
        const uint32_t ob = *reinterpret_cast<const uint32_t *>(lds_raw + sc.lds_fast_order + n * 8u + 4u) >> 16;
        b_in = nb != kNone && ob < seg_hi;
    } else if (nv.in_lds) {
        nb = lds_node_u32(nv.n, 1, n); next = lds_node_u32(nv.n, 2, n);
    } else {
        nb = nv.global[n].b; next = nv.global[n].escape;
    }
    bool second = (w.state & kWalkSecond) != 0;
    for (int c = 0; c < 2; c++) {  // one inlined copy of the test
        bool found;
        if (c == 0 && have_first) {  // the wave has already answered this one together (walk_object_pass)
            found = first_found;
            if (found) {
                best.t = first_t;
                best.ref = first_ref;
                best.obj = ref & kRefIndexMask;
            }
        } else {
            found = leaf_test_kind<T, K>(sc, ref, r, w.a, tmin, w.closest, best, rng PH_PASS);
        }
        if (found) {
            w.any = true;
            w.closest = best.t;
        }
        bool again = !second && nb != ref;
        if constexpr (T::SEG) again = !second && b_in;  // no leaf is held twice in the library's tree, and none is a medium
        else if constexpr (T::MEDIA) again = again || (!second && is_medium_leaf(nb));
        if (!again) {
            w.state = next;
            break;
        }
        if (leaf_kind(nb) != K) {
            w.state = (w.state & ~(3u << kWalkKindShift)) | kWalkSecond | (leaf_kind(nb) << kWalkKindShift);
            break;
        }
        second = true;
        ref = nb;
    }
}

// The LK_OBJECT pass.  A large group of static spheres behind an instance (the Book-2 final scene's 1000-sphere
// cluster) is not walked lane by lane through its sub-BVH in global memory -- a handful of lanes chasing ~50 dependent
// L2 loads each while the other sixty wait -- but scanned by the whole wave, one parked ray at a time: lane l tests
// spheres l, l + 64, ... of the group in object space and a wave-wide minimum over (t, index) picks the hit.  Spheres
// draw no random numbers and the reference's list scan keeps the smallest acceptable root (lowest index on ties), so the
// result is the one HittableList::Hit returns (R/HittableList.h:39-57; the same argument as scan_cooperative's).
// Everything else of this kind (small groups, boxes behind transforms, ...) takes the per-lane test.
DEV double bcast(double x, int src_lane);
DEV void wave_min(double &t, uint32_t &k);
template <class T>
DEV void walk_object_pass(const DeviceScene &sc, const NodeView &nv, const Ray &r, double tmin, Walk &w, HitInfo &best, Xorwow &rng,
                          uint32_t pending, bool mine, uint32_t lane PH_ARG, uint32_t seg_lo = 0u, uint32_t seg_hi = 0u)
{
    ObjectRec o{};
    Ray lr = r;
    o.coop_first = kNone;
    if (mine) {
        o = get_object(sc, pending & kRefIndexMask);
        if (o.coop_first != kNone) lr = to_object_space(sc, o, r);
    }
    const bool coop = mine && o.coop_first != kNone;
    bool found = false;
    double found_t = 0.0;
    uint32_t found_ref = kNone;
    unsigned long long todo = __ballot(coop);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        Ray q;
        q.o = mk(bcast(lr.o.x, src), bcast(lr.o.y, src), bcast(lr.o.z, src));
        q.d = mk(bcast(lr.d.x, src), bcast(lr.d.y, src), bcast(lr.d.z, src));
        const double tmax = bcast(w.closest, src);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)o.coop_first, src);
        const uint32_t count = (uint32_t)__builtin_amdgcn_readlane((int)o.count, src);
        const uint32_t boxes = (uint32_t)__builtin_amdgcn_readlane((int)o.coop_boxes, src);
        const double a = dot(q.d, q.d);
        double bt = tmax;
        uint32_t bk = kNone;
        // Cull by groups of sixteen rows: lane g slab-tests the padded box of group g (R/AABB.h's test, conservative here),
        // then the wave tests only the spheres of the groups the ray passes, four groups (64 spheres) at a time.  A zero
        // direction component would put NaNs into the slab test: such a ray (none in practice) culls nothing.
        const bool axis_parallel = q.d.x == 0.0 || q.d.y == 0.0 || q.d.z == 0.0;
        const Vec inv = mk(1.0 / q.d.x, 1.0 / q.d.y, 1.0 / q.d.z);
        const uint32_t n_groups = (count + kCoopGroup - 1u) / kCoopGroup;
        for (uint32_t g0 = 0; g0 < n_groups; g0 += 64u) {
            const uint32_t g = g0 + lane;
            bool pass = g < n_groups;
            if (pass && !axis_parallel) {
                const GroupBox gb = get_group_box(sc, boxes + g);
                pass = box_test(gb.lo[0], gb.hi[0], gb.lo[1], gb.hi[1], gb.lo[2], gb.hi[2], q, inv, tmin, tmax);
            }
            unsigned long long hits = __ballot(pass);
            while (hits) {
                // the (lane / 16)-th of the next four passing groups is mine
                unsigned long long m = hits;
                int mine_g = -1;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int bit = m ? __ffsll((long long)m) - 1 : -1;
                    if ((int)(lane >> 4) == j) mine_g = bit;
                    m = m ? (m & (m - 1)) : 0ull;
                }
                hits = m;
                const uint32_t k = mine_g >= 0 ? (g0 + (uint32_t)mine_g) * kCoopGroup + (lane & 15u) : count;
                if (k < count) {
                    const SphereGeom sg = get_sphere(sc, first + k);
                    const Vec oc = q.o - mk(sg.cx, sg.cy, sg.cz);
                    const double b = dot(oc, q.d);
                    const double c = dot(oc, oc) - sg.r2;
                    const double disc = b * b - a * c;
                    if (disc > 0.0 && !(tmin >= 0.0 && b > 0.0 && c > 0.0)) {  // see sphere_test
                        double t;
                        if (sphere_roots(b, disc, a, tmin, bt, t)) {
                            bt = t;
                            bk = k;
                        }
                    }
                }
            }
        }
        wave_min(bt, bk);
        if ((int)lane == src) {
            found = bk != kNone;
            found_t = bt;
            found_ref = make_ref(REF_SPHERE, first + bk);
        }
    }
    if (mine) walk_leaf_pass<T, LK_OBJECT>(sc, nv, r, tmin, w, best, rng, pending PH_PASS, coop, found, found_t, found_ref, seg_lo, seg_hi);
}

// Segmented walk: what a ray does between two walks.  Called when the lane has no walk in progress -- a new ray, or the walk
// over the leaf positions [sg.lo, sg.hi) has just ended.  It deals with the world's media in visiting order:
//   * a medium whose padded bounding box the ray does not cross between 0 and the closest hit so far cannot answer:
//     ConstantMedium::Hit clips its two boundary hits to [tMin, tMax] and returns false, before its draw, unless t1 < t2
//     is left (R/ConstantMedium.h:66-71) -- and both boundary hits lie inside the box.  The reference's call would return
//     false without a draw, so the medium is skipped and the surfaces on both sides of it are one segment;
//   * the same when its own boundary queries and clipping, evaluated with the closest hit so far, already say so
//     (object_span + the clipping of R/ConstantMedium.h:66-70; the closest hit can only come nearer, which clips more);
//   * otherwise the surfaces that precede it are walked first, as far as they can matter (their closest hit is the tMax the
//     reference calls the medium with), then the medium is tested -- twice where the reference's span-1 node holds it
//     twice -- with the reference's own arithmetic and draws (object_test);
//   * after the last medium, one walk over the rest of the list.
// The reference reaches a medium only through its BVH, i.e. only if the boxes of the nodes above it are hit within the
// closest hit so far; a medium inside a box the ray misses, or one that lies wholly beyond the closest hit, returns false
// before its draw here as well (no boundary hit, or t1 >= t2 after clipping to tMax), so the draws are the same ones.
template <class T>
DEV void seg_advance(const DeviceScene &sc, const Ray &ray, Walk &w, HitInfo &best, Xorwow &rng, SegState &sg PH_ARG)
{
    uint32_t lo = sg.hi, hi, stage = sg.stage;
    w.closest = w.any ? best.t : DBL_MAX;  // a walk that led up to a medium ran under a lowered bound (below): back to the closest hit itself
    for (;;) {
        if (stage >= sc.n_seg_media) {
            hi = kSegEnd;
            break;
        }
        const SegMedium m = lds_row<SegMedium>(sc.lds_seg_media, stage);
        // its boundary queries (no draw yet): would the call get past its clipping with the closest hit so far?
        bool is_medium;
        MediumRec med{};
        uint32_t medium_index, pref;
        double t1, t2;
        if (!box_test_f(m.fbox[0], m.fbox[1], m.fbox[2], m.fbox[3], m.fbox[4], m.fbox[5], w, 0.0f, w.closest) ||
            !object_span<T, 1>(sc, m.object, ray, 0.001, w.closest, is_medium, med, medium_index, t1, t2, pref PH_PASS) ||
            (t1 < 0.001 ? 0.001 : t1) >= (t2 > w.closest ? w.closest : t2)) {
            stage++;  // it would return false before its draw: no medium here for this ray
            continue;
        }
        // A ray whose stretch that still matters lies inside the medium's box (scattered inside the medium: both ends inside, the box
        // is convex) can only hit the surface leaves that reach into the box: the host has listed them (SegMedium candidates).
        auto inside = [&](Vec p) {
            return p.x >= m.lo[0] && p.x <= m.hi[0] && p.y >= m.lo[1] && p.y <= m.hi[1] && p.z >= m.lo[2] && p.z <= m.hi[2];
        };
        const bool local = m.cand_count != kNone && inside(ray.o);
        // One loop, two trips, so that the candidate tests exist once in the code: trip 0 = the candidates that precede the
        // medium (only when the walk up to it can be skipped), then the medium's draws; trip 1 = all candidates, when the ray
        // ends inside the box after the last medium.
        bool walk_first = false, tested_before = false;
#pragma nounroll
        for (int trip = 0; trip < 2; trip++) {
            const bool here = trip == 0 ? (lo < m.order && local && inside(at(ray, fmin(w.closest, t2))))
                                        : (stage >= sc.n_seg_media && local && w.any && inside(at(ray, w.closest)));
            // trip 0: the candidates before the medium; trip 1: the others -- and those of trip 0 again only if that trip did not run
            // (a leaf answers the same t every time: tested again under a closer bound it can only fall away)
            const uint32_t from = (trip == 1 && tested_before) ? m.order : 0u, below = trip == 0 ? m.order : kSegEnd;
            if (here) {
                for (uint32_t c = 0; c < m.cand_count; c++) {
                    const SegCandidate cd = lds_row<SegCandidate>(sc.lds_seg_cand, m.cand_first + c);
                    if (cd.order < from || cd.order >= below) continue;
                    bool found;
                    if ((cd.ref >> kRefShift) == REF_BOX) {
                        // a box: its two corners first, as a slab test a part in 2^30 wider than the box (the six face planes are the
                        // corner coordinates up to their last bits) -- most candidates end here
                        const BoxRec bx = get_box(sc, cd.ref & kRefIndexMask);
                        const double k30 = 9.313225746154785e-10;
                        const Vec pad = mk(k30 * (fabs(bx.mn[0]) + fabs(bx.mx[0])), k30 * (fabs(bx.mn[1]) + fabs(bx.mx[1])), k30 * (fabs(bx.mn[2]) + fabs(bx.mx[2])));
                        found = box_test(bx.mn[0] - pad.x, bx.mx[0] + pad.x, bx.mn[1] - pad.y, bx.mx[1] + pad.y, bx.mn[2] - pad.z, bx.mx[2] + pad.z, ray,
                                         mk(1.0 / ray.d.x, 1.0 / ray.d.y, 1.0 / ray.d.z), 0.0, w.closest);
                        if (found) {
                            double t;
                            uint32_t face = kNone;
                            found = box_closest(sc, bx, ray, 0.001, w.closest, t, face);
                            if (found) {
                                best.t = t;
                                best.ref = face;
                                best.obj = kNone;
                            }
                        }
                    } else {
                        found = leaf_test_kind<T, LK_PRIM>(sc, cd.ref, ray, w.a, 0.001, w.closest, best, rng PH_PASS);
                    }
                    if (found) {
                        w.any = true;
                        w.closest = best.t;
                    }
                }
                if (trip == 0) tested_before = true;
                else lo = kSegEnd;  // the candidates were all there is left to hit: no walk
            }
            if (trip == 1) break;
            if (lo < m.order && !here) {
                // The surfaces before it first -- but only as far as the medium's far side: the closest hit among them is the tMax
                // of the medium's call, which clips the far boundary hit to it (t2 = min(t2, tMax)); a hit beyond t2 changes
                // nothing there, and the ray's last walk finds it again.
                walk_first = true;
                break;
            }
            for (uint32_t c = 0; c <= m.twice; c++)  // the same two boundary hits every time (geometry), the closest hit as it stands
                if (medium_draw(med.neg_inv_density, medium_index, m.object, ray, 0.001, w.closest, t1, t2, best, rng)) {
                    w.any = true;
                    w.closest = best.t;
                }
            lo = m.order + 1u;
            stage++;
        }
        if (walk_first) {
            hi = m.order;
            w.closest = fmin(w.closest, t2);
            break;
        }
    }
    sg.lo = lo;
    sg.hi = hi;
    sg.stage = stage;
    w.state = (lo < hi && lo < sc.n_world_items) ? 0u : kNone;  // from the root, or nothing to walk
}

// HittableList world (R/HittableList.h:39-57): the item index is wave-uniform, so the primitive rows
// are fetched through the scalar path.
template <class T>
DEV bool world_hit_list(const DeviceScene &sc, const Ray &r, double tmin, double tmax, HitInfo &best, Xorwow &rng PH_ARG)
{
    double a = dot(r.d, r.d);
    double closest = tmax;
    bool any = false;
    const uint32_t n = sc.n_world_items;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t ref = (uint32_t)__builtin_amdgcn_readfirstlane((int)((const RT_CONST uint32_t *)(uintptr_t)sc.world_items)[k]);
        if (leaf_test<T>(sc, ref, r, a, tmin, closest, best, rng PH_PASS)) {
            any = true;
            closest = best.t;
        }
    }
    return any;
}

// HittableList of static spheres (config C2).  Two phases per ray, identical results to the sequential scan:
//  1. convergent scan: every lane evaluates b, c, disc of sphere k (k wave-uniform: the sphere row comes
//     through the scalar cache into SGPRs); a lane for which the reference could accept a root
//     (disc > 0 and not "outside and behind") appends k to its own queue in LDS;
//  2. each lane walks its own queue in ascending k and does the sqrt / divide root selection against its
//     running closest-so-far -- the same order the reference's loop meets those spheres in.
constexpr int kQueueCap = 16;   // entries per lane; the queue is drained whenever a lane could overflow
constexpr int kBurst = 8;           // BVH worlds: at most this many node visits between two leaf phases
constexpr int kRounds = 6;          // node/leaf phase pairs per look at the shading queue, primitive worlds
constexpr int kRoundsComposite = 4; // the same for composite worlds
constexpr int kRoundsFast = 4;      // and for the library-tree kernel, whose frame ends with its long pixels: they are shaded sooner
                                    // (C3, one call: 2 rounds 2615, 3: 2711, 4: 2891-2943, 5: 2805, 6: 2784, 8: 2675 Msamples/s)

DEV void drain_queue(const SphereGeom *__restrict__ spheres, const uint16_t *queue, uint32_t lane, uint32_t &count,
                     const Ray &r, double a, double tmin, double &closest, uint32_t &best_k)
{
    for (uint32_t s = 0; s < count; s++) {
        uint32_t k = queue[s * 64u + lane];
        SphereGeom g = spheres[k];
        Vec oc = r.o - mk(g.cx, g.cy, g.cz);
        double b = dot(oc, r.d);
        double c = dot(oc, oc) - g.r2;
        double disc = b * b - a * c;
        double t;
        if (sphere_roots(b, disc, a, tmin, closest, t)) {
            closest = t;
            best_k = k;
        }
    }
    count = 0;
}

// Four spheres of the convergent scan: the four discriminant chains are independent straight-line code
// (the scheduler interleaves them), then each lane queues the spheres for which a root could be accepted.
DEV void scan_four(const SphereGeom &g0, const SphereGeom &g1, const SphereGeom &g2, const SphereGeom &g3, uint32_t k0,
                   const Ray &r, double a, uint16_t *queue, uint32_t lane, uint32_t &count)
{
    const SphereGeom *g[4] = {&g0, &g1, &g2, &g3};
    double b[4], c[4], disc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        Vec oc = r.o - mk(g[u]->cx, g[u]->cy, g[u]->cz);
        b[u] = dot(oc, r.d);
        c[u] = dot(oc, oc) - g[u]->r2;
        disc[u] = b[u] * b[u] - a * c[u];
    }
    // Pin the four chains ahead of the branches: without this the compiler sinks each chain next to its own branch
    // and a wave executes them one after another, every fp64 op waiting for the previous one's result.
    asm volatile("" : "+v"(disc[0]), "+v"(disc[1]), "+v"(disc[2]), "+v"(disc[3]));
    asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (disc[u] > 0.0 && !(b[u] > 0.0 && c[u] > 0.0)) {  // tmin = 0.001 >= 0: see sphere_test
            queue[count * 64u + lane] = (uint16_t)(k0 + u);
            count++;
        }
    }
}

DEV void scan_one(const SphereGeom &g, uint32_t k, const Ray &r, double a, uint16_t *queue, uint32_t lane, uint32_t &count)
{
    Vec oc = r.o - mk(g.cx, g.cy, g.cz);
    double b = dot(oc, r.d);
    double c = dot(oc, oc) - g.r2;
    double disc = b * b - a * c;
    if (disc > 0.0 && !(b > 0.0 && c > 0.0)) {
        queue[count * 64u + lane] = (uint16_t)k;
        count++;
    }
}

// A no-op that *uses* four scalar rows: it makes the compiler place the wait for those rows here, i.e. before
// the next batch of scalar loads is issued.  (Scalar loads return out of order, so every wait is lgkmcnt(0); a wait
// placed after the next loads were issued would also wait for them and undo the prefetch.)
DEV void rows_arrived(const SphereGeom &g0, const SphereGeom &g1, const SphereGeom &g2, const SphereGeom &g3)
{
    asm volatile("" ::"s"(g0.cx), "s"(g0.cy), "s"(g0.cz), "s"(g0.r2), "s"(g1.cx), "s"(g1.cy), "s"(g1.cz), "s"(g1.r2));
    asm volatile("" ::"s"(g2.cx), "s"(g2.cy), "s"(g2.cz), "s"(g2.r2), "s"(g3.cx), "s"(g3.cy), "s"(g3.cz), "s"(g3.r2));
}

// ---- conservative filter of the list scan -------------------------------------------------------------------------
// The reference tests a ray against a sphere with b = oc.d, c = oc.oc - r^2, disc = b*b - a*c (R/Sphere.h:28-41): 13
// fp64 instructions with the compare, for every sphere of the list, and all but a few per ray end at `disc > 0` false.
// Those are only *rejections*, so they need not be computed the reference's way -- any test that never rejects a sphere
// the reference would accept leaves the image bit for bit the same, as long as the survivors then go through the
// reference's arithmetic (drain_queue).  With u = d/|d|, od = o.u, p = o - od u (the ray's foot point) and, per sphere,
// K = |C|^2 - r^2 (host, scene_builder.cpp):
//     disc / a  =  ((o-C).u)^2 - (|o-C|^2 - r^2)  =  (C.u)^2 + 2 p.C - K  -  (o.o - od^2)
// i.e. Q = fma(s, s, t) with s = C.u (3 instructions), t = 2p.C - (o.o - od^2) (3 fma), compared with the sphere's K: 8
// instructions (the per-ray term is the addend that opens the chain and K is an operand of the compare: either as an
// addend of its own would cost a move from the scalar row into a vector register).
// Rounding: every term above is at most W^2 in magnitude, W = |o| + max(|C| + r) (`scan_reach`); the 8 operations, the
// rounding of u (three divisions and a square root, so u is neither exactly unit nor exactly parallel to d), of K, p and
// od, and the reference's own rounding of disc (divided by a) each move the comparison by at most a few u W^2,
// u = 2^-53; their sum is below 64 u W^2.  The filter lowers the threshold by M = 2^-40 W^2 (8192 u W^2): it passes
// whenever the reference's disc, however rounded, is positive, and a sphere of radius r is passed in vain only by rays
// that miss it by less than M / 2r (4e-6 W^2 / r world units^2: for config C2, W = 2013, a band of 1e-5 of a small
// sphere's radius).  A ray with a non-finite or vanishing direction passes every sphere (u = p = 0, addend +inf).
// The reference's second shortcut -- the sphere is behind an outside origin, sphere_test -- is applied to the survivors
// with the same margin: bu = od - s > sqrt(M) and bu^2 - disc/a > M imply b > 0 and c > 0 in the reference's arithmetic.
struct ScanRay {
    Vec u, p2;           // d / |d|,  2 (o - (o.u) u)
    double nthr;         // M - (o.o - (o.u)^2)
    double od, root_m;   // o.u,  sqrt(M)
};
DEV ScanRay scan_ray(const Ray &r, double a, double reach)
{
    ScanRay f;
    const double oo = dot(r.o, r.o);
    const double w = sqrt(oo) + reach;
    const bool sane = a > 1e-280 && a < 1e280 && w < 1e140;
    if (sane) {
        const double inv = 1.0 / sqrt(a);
        f.u = inv * r.d;
        f.od = dot(r.o, f.u);
        f.p2 = 2.0 * (r.o - f.od * f.u);
        f.root_m = 0x1p-20 * w;
        f.nthr = f.root_m * f.root_m - (oo - f.od * f.od);
    } else {
        f.u = f.p2 = mk(0.0, 0.0, 0.0);
        f.od = 0.0;
        f.root_m = __builtin_inf();
        f.nthr = __builtin_inf();
    }
    return f;
}
DEV double filter_s(const ScanRay &f, double cx, double cy, double cz)
{
    return __builtin_fma(cz, f.u.z, __builtin_fma(cy, f.u.y, cx * f.u.x));
}
DEV double filter_q(const ScanRay &f, double s, double cx, double cy, double cz)  // the sphere passes when this exceeds its K
{
    return __builtin_fma(s, s, __builtin_fma(f.p2.z, cz, __builtin_fma(f.p2.y, cy, __builtin_fma(f.p2.x, cx, f.nthr))));
}
DEV bool filter_behind(const ScanRay &f, double s, double q, double k)  // only for a sphere that passed: q > k
{
    const double bu = f.od - s;
    return bu > f.root_m && __builtin_fma(bu, bu, k - q) > 0.0;
}

DEV SphereScanRow load_scan_row(const SphereScanRow *table, uint32_t k)
{
    const RT_CONST double *p = const_doubles(table + k);
    return SphereScanRow{p[0], p[1], p[2], p[3]};
}
DEV void scan_rows_arrived(const SphereScanRow &g0, const SphereScanRow &g1, const SphereScanRow &g2, const SphereScanRow &g3)
{
    asm volatile("" ::"s"(g0.cx), "s"(g0.cy), "s"(g0.cz), "s"(g0.k), "s"(g1.cx), "s"(g1.cy), "s"(g1.cz), "s"(g1.k));
    asm volatile("" ::"s"(g2.cx), "s"(g2.cy), "s"(g2.cz), "s"(g2.k), "s"(g3.cx), "s"(g3.cy), "s"(g3.cz), "s"(g3.k));
}

// Append sphere k to this lane's queue if `keep`.  Called for a sphere that some lane of the wave passed (a wave-uniform
// branch on the ballot of the pass bits, so a sphere no lane passed costs no vector instruction): every lane writes its
// next slot and only the lanes that keep the sphere move `count` on, so the append needs no exec mask of its own.  A slot
// written in vain is overwritten by the lane's next append or lies beyond `count`, where the drain does not read; it is
// always inside the queue: the scans drain before any lane could hold kQueueCap entries, so count < kQueueCap here.
// Primary rounds (render_kernel; primary_cull_rule.h): when a round of list tests pays.  A round costs the wave its own
// instructions, and a lane it takes out of the next pixel-parallel pass saves 1/64 of that pass.  Census of the built kernel
// (DESIGN.md section 4 "(r18)"), vector instructions: a round is about 735 (30 to decide, 55 per trip of the entry loop and 5
// trips for the fullest lane, 400 of shading and the next camera ray, 30 at the loop's head); a pass is about 1200 whatever
// the list (survivors, drain, set-up, shading) plus 3.54 per sphere of the list (1716 for C2's 485).  The break-even number of
// fresh lanes is 64 x 735 / (1200 + 3.54 n): 16 for C2, 34 for a list of 50, 39 at most.
// A round also delays every secondary ray of its wave.  For a pixel whose chain of rays is what the frame waits for, that is
// pure loss: a wave holding a pixel that has traced more than kPrimaryLongChain rays per sample (over at least 16 samples'
// worth) runs no round that leaves a lane waiting.  C2's mean is 2.3 rays per sample; the serving threshold is 9.
constexpr uint32_t kPrimaryRoundCost = 735, kPrimaryPassFixed = 1200, kPrimaryPassPerSphere100 = 354;
constexpr uint32_t kPrimaryLongChain = 6;
constexpr int kFilterTrip = 8;  // spheres per trip of the filtered scans; they drain when a lane holds more than kQueueCap - kFilterTrip
static_assert(kFilterTrip < kQueueCap, "a trip of appends must fit between the drain threshold and the end of the queue");
DEV void append_survivor(uint16_t *queue, uint32_t lane, uint32_t &count, uint32_t k, bool keep)
{
    queue[count * 64u + lane] = (uint16_t)k;
    count += keep ? 1u : 0u;
}

// Four spheres through the filter: four independent chains, one wave-level branch for the four of them, then one per sphere
// that some lane passed.
DEV void filter_four(const SphereScanRow &g0, const SphereScanRow &g1, const SphereScanRow &g2, const SphereScanRow &g3, uint32_t k0,
                     const ScanRay &f, uint16_t *queue, uint32_t lane, uint32_t &count)
{
    const SphereScanRow *g[4] = {&g0, &g1, &g2, &g3};
    double s[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        s[u] = filter_s(f, g[u]->cx, g[u]->cy, g[u]->cz);
        q[u] = filter_q(f, s[u], g[u]->cx, g[u]->cy, g[u]->cz);
    }
    asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]));
    const bool p[4] = {q[0] > g0.k, q[1] > g1.k, q[2] > g2.k, q[3] > g3.k};
    const unsigned long long m[4] = {__ballot(p[0]), __ballot(p[1]), __ballot(p[2]), __ballot(p[3])};  // the compares' own lane masks
    if (m[0] | m[1] | m[2] | m[3]) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!m[u]) continue;  // wave-uniform: no lane passed this sphere
            const bool keep = p[u] && !filter_behind(f, s[u], q[u], g[u]->k);
            append_survivor(queue, lane, count, k0 + u, keep);
        }
    }
}

// drain_queue for survivors of the filter: the reference's whole test, `disc > 0` included.  ROWS_IN_LDS: the rows come
// from the LDS planes of the cooperative scan (a queue entry costs one LDS round trip instead of one to L2).
template <bool ROWS_IN_LDS>
DEV void drain_filtered(const SphereGeom *__restrict__ spheres, uint32_t planes_off, uint32_t n_padded, const uint16_t *queue, uint32_t lane,
                        uint32_t &count, const Ray &r, double a, double tmin, double &closest, uint32_t &best_k SS_ARG)
{
#if RT_PHASES
    const unsigned long long ss_t0 = __builtin_readcyclecounter();
    uint32_t ss_max = count;
    for (int off = 32; off > 0; off >>= 1) ss_max = max(ss_max, (uint32_t)__shfl_xor((int)ss_max, off, 64));
    ss.drains++;
    ss.drain_iters += ss_max;
#endif
    for (uint32_t s = 0; s < count; s++) {
        uint32_t k = queue[s * 64u + lane];
        SphereGeom g;
        if constexpr (ROWS_IN_LDS) {
            const RT_LDS double *pl = (const RT_LDS double *)(lds_raw + planes_off);
            g = SphereGeom{pl[k], pl[n_padded + k], pl[2u * n_padded + k], pl[3u * n_padded + k]};
        } else {
            g = spheres[k];
        }
        double t;
        if (sphere_test(r.o - mk(g.cx, g.cy, g.cz), r.d, a, g.r2, tmin, closest, t)) {
            closest = t;
            best_k = k;
        }
    }
    count = 0;
#if RT_PHASES
    asm volatile("" ::"v"(closest), "v"(best_k));
    ss.drain_cycles += (uint32_t)(__builtin_readcyclecounter() - ss_t0);
#endif
}

// ---- the same filter in packed fp32, two spheres per instruction (r3) -------------------------------------------------------
// gfx950 issues v_pk_fma_f32 (two fp32 fmas per lane) in the slot of one v_fma_f64, so the filter's seven multiply-adds cost
// 7 instructions per PAIR of spheres plus two compares: 4.5 per sphere instead of 8.  It only ever rejects, so it may be as
// coarse as fp32 makes it as long as it never rejects what the reference accepts.  Error of the computed Q against the exact
// disc / a + K + M (same quantities as above, everything rounded to fp32 -- centre, u, 2p, the per-ray addend, every product
// and sum): at most 2^-24 (17 W^2 + 5 M) with W = |o| + max |C| over the spheres this filter DECIDES (`scan_reach32`: the bulk
// of the list; a sphere far outside it, like the Book-1 ground sphere, has k = -inf and always goes on to the exact test),
// plus 2^-24 W^2 for the rounding of K.  With M = 2^-18 W^2 (64 x 2^-24 W^2) the threshold is lowered 3.5 times that:
// a sphere the reference could accept always passes; a sphere is passed in vain by rays that miss it by less than
// M / 2r (C2: W = 30, M = 3.4e-3, 4 % of a small sphere's radius).  The behind-the-origin shortcut keeps its form with
// the fp32 margins (bu > 2^-9 W >> its own error 2^-21 W; bu^2 - disc/a > M).  tests/test_filter_margin.py restates both
// forms operation by operation.
// The RUN form (r13; flat_scene.h ScanSegment): over a range of rows whose centres share the fp32 coordinate c on one axis, say y,
//     s0 = fl(c uy),  l0 = fl(py c + nt)                  once per ray and segment
//     s = fma(cz, uz, fma(cx, ux, s0)),  Q = fma(s, s, fma(pz, cz, fma(px, cx, l0)))
// is the general form with its sums taken in another order: the same seven products of the same rounded operands, and the same
// seven roundings -- three on the way to s (s0 takes the place of the opening product cx ux), four on the way to Q (l0 takes the
// place of the opening fma on nt) -- each of a partial sum of the same terms.  The bound above never used the order: it charges
// every rounding 2^-24 of the largest partial sum it can meet, W |u| <= W for s and W^2 + M for the chain of Q (|2 p.C| <= 2 W^2
// only with all three products in; any subset is no larger than 2 |p| |C|), and s enters Q through s^2 <= W^2 with twice its
// relative error.  So the run form's error is at most the same 2^-24 (17 W^2 + 5 M), the margin M = 2^-18 W^2, root_m, nthr and
// `scan_reach32` stay as they are, and c -- the bit-same fp32 value the rows would have held -- is rounded once, on the host, as
// every centre coordinate is.  Rows with k = -inf / +inf keep zeros for a centre: their s = s0 and Q = s0^2 + l0 are finite (or
// +inf for a degenerate ray), never NaN, so they pass always / never as in the general form.  tests/test_filter_shared_axis.py
// restates the run form the same way.
typedef float v2f __attribute__((ext_vector_type(2)));
struct ScanRay32 {
    float ux, uy, uz, px, py, pz;  // d / |d|,  2 (o - (o.u) u)
    float nthr;                    // M - (o.o - (o.u)^2)
    float od, root_m;              // o.u,  sqrt(M)
};
DEV ScanRay32 scan_ray32(const Ray &r, double a, double reach)
{
    ScanRay32 f;
    const double oo = dot(r.o, r.o);
    const double w = sqrt(oo) + reach;
    const bool sane = a > 1e-280 && a < 1e280 && w < 1e15;
    if (sane) {
        const double inv = 1.0 / sqrt(a);
        const Vec u = inv * r.d;
        const double od = dot(r.o, u);
        const Vec p2 = 2.0 * (r.o - od * u);
        const double root_m = 0x1p-9 * w;
        f.ux = (float)u.x; f.uy = (float)u.y; f.uz = (float)u.z;
        f.px = (float)p2.x; f.py = (float)p2.y; f.pz = (float)p2.z;
        f.od = (float)od;
        f.root_m = (float)root_m;
        f.nthr = (float)(root_m * root_m - (oo - od * od));
    } else {  // a degenerate ray passes every sphere and none is called behind
        f.ux = f.uy = f.uz = f.px = f.py = f.pz = f.od = 0.0f;
        f.root_m = __builtin_inff();
        f.nthr = __builtin_inff();
    }
    return f;
}
// One pair of rows at `byte_off + ahead` past `table` (the sum is formed in 64 bits: `ahead`, a constant, then becomes the load's
// immediate offset and `byte_off` its register offset, with no addition in the loop), which the host pads (scene_builder.cpp kScanTripPairs) so that a whole trip and the
// prefetch behind it stay inside it.  The load is volatile: an ordinary scalar load is sunk to its first use, which puts the loads
// of a trip's second half directly in front of the wait that retires them; a volatile one keeps its place among the branches, half
// a trip of filter arithmetic ahead of its wait.  It is still one s_load_dwordx8 from the (immutable) table.
typedef float v8f __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
DEV SphereScanPair load_scan_pair(const SphereScanPair *table, uint32_t byte_off, uint32_t ahead)
{
    const RT_CONST char *p = ((const RT_CONST char *)(uintptr_t)table + byte_off) + ahead;
    const v8f v = *(const volatile RT_CONST v8f *)p;
    return SphereScanPair{{v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}, {v[6], v[7]}};
}
DEV void scan_pairs_arrived(const SphereScanPair &g0, const SphereScanPair &g1)
{
    asm volatile("" ::"s"(g0.cx[0]), "s"(g0.cx[1]), "s"(g0.cy[0]), "s"(g0.cy[1]), "s"(g0.cz[0]), "s"(g0.cz[1]), "s"(g0.k[0]), "s"(g0.k[1]));
    asm volatile("" ::"s"(g1.cx[0]), "s"(g1.cx[1]), "s"(g1.cy[0]), "s"(g1.cy[1]), "s"(g1.cz[0]), "s"(g1.cz[1]), "s"(g1.k[0]), "s"(g1.k[1]));
}
// The ray's side of the packed filter: every term twice, once per sphere of a pair.
struct ScanRayPairs {
    v2f ux, uy, uz, px, py, pz, nt;
    float od, root_m;
};
DEV ScanRayPairs scan_ray_pairs(const ScanRay32 &f)
{
    return ScanRayPairs{{f.ux, f.ux}, {f.uy, f.uy}, {f.uz, f.uz}, {f.px, f.px}, {f.py, f.py}, {f.pz, f.pz}, {f.nthr, f.nthr}, f.od, f.root_m};
}
// A no-op that the two operands which open the filter's chains pass THROUGH.  Placed behind the loads of the other register set
// it keeps the filter's arithmetic behind those loads (they are volatile and it is an asm volatile: their order holds), so the
// loads are issued at the head of their half of the trip and not wherever the scheduler drops them among the arithmetic.
DEV void filter_starts_here(v2f &opens_s, v2f &opens_q)
{
    asm volatile("" : "+v"(opens_s), "+v"(opens_q));
}
// One segment of the table's trips (flat_scene.h ScanSegment), read on the scalar path: one s_load_dwordx4 per segment.
DEV ScanSegment load_scan_segment(const ScanSegment *table, uint32_t k)
{
    const RT_CONST uint32_t *p = (const RT_CONST uint32_t *)(uintptr_t)(table + k);
    return ScanSegment{p[0], p[1], p[2], __builtin_bit_cast(float, p[3])};
}
// Two pairs = four spheres (list positions k0 .. k0 + 3): two packed chains, four compares, one wave-level branch for the four of
// them, then the survivor path only for the spheres some lane passed (as in filter_four).  `earlier` is the ballot of what the
// same trip passed before these four; the return value adds these four's to it.  The one branch is taken when either is non-zero,
// and `after_appends` (the caller's drain test: see scan_filtered32) runs behind that same branch, so a trip in which no lane
// passed anything executes two compares and two branches not taken for its eight spheres.
// RUN: the rows of a run segment -- cx and cz slots hold the two varying coordinates, f.ux / f.uz / f.px / f.pz the ray's terms
// for them, s0 = c u and l0 = fma(p, c, nt) the shared coordinate's share of both chains (scan_filtered32): five packed
// instructions per pair instead of seven.  Otherwise s0 and l0 are not read.
template <bool RUN, class AFTER>
DEV unsigned long long filter_pairs(const SphereScanPair &g0, const SphereScanPair &g1, uint32_t k0, const ScanRayPairs &f, v2f s0, v2f l0, uint16_t *queue,
                                    uint32_t lane, uint32_t &count, unsigned long long earlier, AFTER &&after_appends SS_ARG)
{
    const v2f ux = f.ux, uy = f.uy, uz = f.uz, px = f.px, py = f.py, pz = f.pz, nt = f.nt;
    const SphereScanPair *g[2] = {&g0, &g1};
    v2f s[2], q[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const v2f cx = {g[h]->cx[0], g[h]->cx[1]}, cy = {g[h]->cy[0], g[h]->cy[1]}, cz = {g[h]->cz[0], g[h]->cz[1]};
        if constexpr (RUN) {
            s[h] = __builtin_elementwise_fma(cz, uz, __builtin_elementwise_fma(cx, ux, s0));
            q[h] = __builtin_elementwise_fma(s[h], s[h], __builtin_elementwise_fma(pz, cz, __builtin_elementwise_fma(px, cx, l0)));
        } else {
            s[h] = __builtin_elementwise_fma(cz, uz, __builtin_elementwise_fma(cy, uy, cx * ux));
            q[h] = __builtin_elementwise_fma(s[h], s[h], __builtin_elementwise_fma(pz, cz, __builtin_elementwise_fma(py, cy, __builtin_elementwise_fma(px, cx, nt))));
        }
    }
    const bool p[4] = {q[0].x > g0.k[0], q[0].y > g0.k[1], q[1].x > g1.k[0], q[1].y > g1.k[1]};
    const unsigned long long m[4] = {__ballot(p[0]), __ballot(p[1]), __ballot(p[2]), __ballot(p[3])};  // the compares' own lane masks
    const unsigned long long mine = m[0] | m[1] | m[2] | m[3];
#if RT_PHASES
    ss.groups++;
    ss.taken += mine ? 1u : 0u;
    ss.spheres += (m[0] ? 1u : 0u) + (m[1] ? 1u : 0u) + (m[2] ? 1u : 0u) + (m[3] ? 1u : 0u);
#endif
    const unsigned long long all = mine | earlier;
    if (__builtin_expect(all != 0, 0)) {
        const float sv[4] = {s[0].x, s[0].y, s[1].x, s[1].y}, qv[4] = {q[0].x, q[0].y, q[1].x, q[1].y};
        const float kv[4] = {g0.k[0], g0.k[1], g1.k[0], g1.k[1]};
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (!m[u]) continue;  // wave-uniform: no lane passed this sphere
            const float bu = f.od - sv[u];
            const bool behind = bu > f.root_m && __builtin_fmaf(bu, bu, kv[u] - qv[u]) > 0.0f;  // k = -inf (always passes): never behind
#if RT_PHASES
            ss.appends += (uint32_t)__popcll(__ballot(p[u] && !behind));
            ss.behind += (uint32_t)__popcll(__ballot(p[u] && behind));
#endif
            append_survivor(queue, lane, count, k0 + u, p[u] && !behind);
        }
        after_appends();
    }
    return all;
}

// One trip of the packed scan at byte offset `off`, in the general or the run form; the loads, their waits and the branches are the
// same in both.  `opens_s` / `opens_q` are the operands that open the filter's two chains: s0 and l0 of the run segment, or the
// ray's own ux and nt in the general form (which filter_pairs<false> reads from `f`).  There they alias members of `f` on purpose:
// it is what ties filter_starts_here to the very registers the general chains open with.
template <bool RUN, bool ROWS_IN_LDS>
DEV void scan_trip(const SphereScanPair *__restrict__ rows, const SphereGeom *__restrict__ spheres, uint32_t &off, uint32_t &end, SphereScanPair &a0,
                   SphereScanPair &a1, const ScanRayPairs &f, v2f &opens_s, v2f &opens_q, uint32_t planes_off, uint32_t n_padded, uint16_t *queue, uint32_t lane,
                   uint32_t &count, const Ray &r, double a, double tmin, double &closest, uint32_t &best_k SS_ARG)
{
    constexpr uint32_t kPairBytes = (uint32_t)sizeof(SphereScanPair), kTripBytes = kScanTripPairs * kPairBytes;
    const uint32_t k0 = off / (kPairBytes / 2u);  // sphere index of the trip: used on the survivor path only
    scan_pairs_arrived(a0, a1);
    const SphereScanPair b0 = load_scan_pair(rows, off, 2u * kPairBytes), b1 = load_scan_pair(rows, off, 3u * kPairBytes);
    filter_starts_here(opens_s, opens_q);
    const unsigned long long passed = filter_pairs<RUN>(a0, a1, k0, f, opens_s, opens_q, queue, lane, count, 0ull, [] {} SS_PASS);
    scan_pairs_arrived(b0, b1);
    a0 = load_scan_pair(rows, off, 4u * kPairBytes);  // the next trip's (of whichever segment), or the padding behind the last one
    a1 = load_scan_pair(rows, off, 5u * kPairBytes);
    filter_starts_here(opens_s, opens_q);
    filter_pairs<RUN>(b0, b1, k0 + 4u, f, opens_s, opens_q, queue, lane, count, passed, [&] {
        if (__any(count > (uint32_t)(kQueueCap - kFilterTrip))) drain_filtered<ROWS_IN_LDS>(spheres, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
    } SS_PASS);
    off += kTripBytes;
    asm volatile("" : "+s"(off), "+s"(end));  // the loop's own two registers: every mention weighs against spilling them
}
DEV void scan_swap(v2f &a, v2f &b) { const v2f t = a; a = b; b = t; }
// Pixel-parallel scan through the packed fp32 filter: pairs of sphere rows are wave-uniform (scalar path), four pairs (eight
// spheres) per trip in two register sets like scan_filtered; the survivors go through drain_filtered, i.e. the reference's test.
// The table is padded to whole trips with rows that never pass, plus the two pairs the last trip prefetches (kScanTripPairs,
// kScanAheadPairs), so the loop has no tail and no clamp: its only state is the byte offset of the trip, from which the survivor
// path derives the sphere index.
// Queue bound: `count` changes only in append_survivor.  At the head of a trip every lane holds at most kQueueCap - kFilterTrip
// entries: true at the start, kept by a trip that appends nothing, and restored by the drain test that follows every trip in
// which some lane passed a sphere.  A trip appends at most kFilterTrip entries per lane, so a lane writes its slot `count` only
// while count < kQueueCap.
//
// Windows (r29; scan_window_rule.h), the WINDOWS instantiation: a launch takes it where some run of the scene has a window table and
// RT_FLAG_NO_SCAN_WINDOWS is not set; every other launch takes the other instantiation, which is the scan as it was before r29,
// called by the live lanes only.  With WINDOWS all 64 lanes come here and `live` says which of them hold a ray: the others get
// a filter addend of -inf, so that their Q is -inf or NaN and passes no row (k = -inf included: -inf > -inf is false); they
// append nothing and drain nothing, and every ballot, the drain test's too, is what it is when only the live lanes come.  In a
// run whose window record names an axis (the records lie behind the segment records, the spans behind those: no pointer of
// their own is carried through the loops) every lane forms the extent of its ray on that axis inside the run's slab, the wave
// unites them (two DPP reductions), lane t tests trip t of a chunk of 64 against the union, and the ballot, its short gaps
// filled, is the set of trips to run: `off` and `end` are set per range of set bits, set A is read afresh where `off` jumps,
// and behind the run `off` stands at its end with set A of whatever follows.  The spans are read from their LDS copy where the
// launch staged one (with the sphere planes: launch_plan.cpp lds_layout), else from global memory: 8 bytes a lane, one read a
// chunk, issued ahead of the extents' arithmetic.  A run without a table keeps
// the loop it had, in a copy of its own.  A range comes from set bits of lanes below the chunk's number of trips and nowhere
// else, so first <= last < n_trips, and a range is never empty: the loop's `off != end` test is reached with off < end only.
// Survivors reach the queues in ascending list position as before, and the queue bound above holds verbatim.
DEV ScanWindowSeg load_scan_window(const ScanWindowSeg *table, uint32_t k)
{
    const RT_CONST uint32_t *p = (const RT_CONST uint32_t *)(uintptr_t)(table + k);
    return ScanWindowSeg{p[0], __builtin_bit_cast(float, p[1]), __builtin_bit_cast(float, p[2]), p[3]};
}
// The span of trip t: from the LDS copy where the launch staged one (launch_plan.cpp lds_layout), else from behind the segment records.
DEV ScanTripSpan load_scan_span(const DeviceScene &sc, uint32_t t)
{
    if (sc.lds_scan_spans != kNone && sc.lds_scan_spans != 0u) {
        const v2f v = *(const RT_LDS v2f *)(lds_raw + sc.lds_scan_spans + t * (uint32_t)sizeof(ScanTripSpan));
        return ScanTripSpan{v.x, v.y};
    }
    return reinterpret_cast<const ScanTripSpan *>(sc.scan_segments + 2u * sc.n_scan_segments)[t];
}
template <int CTRL, int ROW_MASK>
DEV void fmin_step(float &x, float &y)
{
    const float ox = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, false));
    const float oy = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, y), __builtin_bit_cast(int, y), CTRL, ROW_MASK, 0xf, false));
    x = __builtin_fminf(x, ox);
    y = __builtin_fminf(y, oy);
}
// Wave-wide minimum of x and of y (neither is ever NaN), as scalars: the steps of wave_min.  All 64 lanes must be enabled.
DEV void wave_fmin2(float &x, float &y)
{
    fmin_step<0xB1, 0xf>(x, y);
    fmin_step<0x4E, 0xf>(x, y);
    fmin_step<0x114, 0xf>(x, y);
    fmin_step<0x118, 0xf>(x, y);
    fmin_step<0x142, 0xa>(x, y);
    fmin_step<0x143, 0xc>(x, y);
    x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
    y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), 63));
}
template <bool ROWS_IN_LDS, bool WINDOWS>
DEV bool scan_filtered32(const DeviceScene &sc, bool live, uint32_t planes_off, uint32_t n_padded, uint16_t *queue, uint32_t lane,
                         const Ray &r, double tmin, double tmax, HitInfo &best SS_ARG)
{
    static_assert(kFilterTrip == 2 * kScanTripPairs && kScanAheadPairs == 2, "one trip = four pairs in two halves; set A of the next trip is read ahead");
    constexpr uint32_t kPairBytes = (uint32_t)sizeof(SphereScanPair), kTripBytes = kScanTripPairs * kPairBytes;
    const SphereScanPair *__restrict__ rows = sc.sphere_scan32;
    const ScanSegment *__restrict__ segments = sc.scan_segments;
    const SphereGeom *__restrict__ spheres = sc.spheres;
    const uint32_t n_segments = sc.n_scan_segments;  // they tile the table's trips in order (scene_builder.cpp cut_scan_segments)
    const double a = dot(r.d, r.d);
    ScanRayPairs f = scan_ray_pairs(scan_ray32(r, a, sc.scan_reach32));
    if constexpr (WINDOWS)
        if (!live) f.nt = v2f{-__builtin_inff(), -__builtin_inff()};
    double closest = tmax;
    uint32_t best_k = kNone, count = 0;
    if (n_segments) {
        SphereScanPair a0 = load_scan_pair(rows, 0u, 0u), a1 = load_scan_pair(rows, 0u, kPairBytes);
        uint32_t off = 0, end = 0;
        for (uint32_t seg = 0; seg != n_segments; seg++) {
            const ScanSegment sg = load_scan_segment(segments, seg);
            end = (sg.first_trip + sg.n_trips) * kTripBytes;  // off stands at sg.first_trip * kTripBytes: the segments tile the trips
            if (sg.axis == kScanAxisNone) {
                do scan_trip<false, ROWS_IN_LDS>(rows, spheres, off, end, a0, a1, f, f.ux, f.nt, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
                while (off != end);
            } else {
                const uint32_t seg_end = end;
                bool windowed = false;  // the run has a window table, and x0, x1 hold the wave's window
                float x0 = 0.0f, x1 = 0.0f;  // the union of the wave's extents on the window axis
                uint32_t chunk = sg.first_trip;  // the first trip of the chunk of 64 that `need` speaks of
                unsigned long long need = 0;     // that chunk's trips still to run
                if constexpr (WINDOWS) {
                    // the window records lie directly behind the segment records, the spans behind those (device_scene.cpp rt_scene_upload)
                    const ScanWindowSeg *windows = reinterpret_cast<const ScanWindowSeg *>(segments + n_segments);
                    const ScanWindowSeg ws = load_scan_window(windows, seg);
                    const uint32_t window_axis = ws.axis;
                    windowed = window_axis != kScanAxisNone;
                    if (windowed) {
#if RT_PHASES
                        const unsigned long long ss_w0 = __builtin_readcyclecounter();
#endif
                        // lane t's trip of the run's first chunk, read ahead of the extents' arithmetic
                        const bool in_run = lane < sg.n_trips;
                        ScanTripSpan sp{0.0f, 0.0f};
                        if (in_run) sp = load_scan_span(sc, sg.first_trip + lane);
                        float e0 = __builtin_inff(), e1 = __builtin_inff();  // min of lo, min of -hi: no ray, the empty extent
                        if (live) {
                            const double oa = sg.axis == 0u ? r.o.x : (sg.axis == 1u ? r.o.y : r.o.z), da = sg.axis == 0u ? r.d.x : (sg.axis == 1u ? r.d.y : r.d.z);
                            const double ow = window_axis == 0u ? r.o.x : (window_axis == 1u ? r.o.y : r.o.z), dw = window_axis == 0u ? r.d.x : (window_axis == 1u ? r.d.y : r.d.z);
                            const ScanExtent ex = scan_window_extent(oa, da, ow, dw, __builtin_fabs(r.o.x) + __builtin_fabs(r.o.y) + __builtin_fabs(r.o.z), a, sc.scan_reach32, (double)ws.slab_lo, (double)ws.slab_hi);
                            e0 = (float)ex.lo;
                            e1 = -(float)ex.hi;
                        }
#if RT_PHASES
                        const float own0 = e0, own1 = -e1;  // this lane's own extent (no ray: empty)
#endif
                        wave_fmin2(e0, e1);
                        x0 = e0;
                        x1 = -e1;
                        need = scan_window_fill(__ballot(in_run && scan_window_needs(sp.lo, sp.hi, x0, x1)));
#if RT_PHASES
                        asm volatile("" ::"s"(x0), "s"(x1));
                        ss.win_cycles += (uint32_t)(__builtin_readcyclecounter() - ss_w0);
                        ss.win_runs++;
                        for (uint32_t t = 0; t < sg.n_trips; t++) {  // outside the cycle count: what each lane's own extent needs of the run
                            const ScanTripSpan own = load_scan_span(sc, sg.first_trip + t);
                            ss.win_lane_trips += (uint32_t)__popcll(__ballot(live && scan_window_needs(own.lo, own.hi, own0, own1)));
                        }
#endif
                    }
                }
                // The ray's terms for the run's two varying coordinates go where the rows keep those (flat_scene.h ScanSegment),
                // the shared coordinate's to the middle slot, and back behind the run.
                if (sg.axis == 0u) { scan_swap(f.ux, f.uy); scan_swap(f.px, f.py); }
                if (sg.axis == 2u) { scan_swap(f.uz, f.uy); scan_swap(f.pz, f.py); }
                const v2f c = {sg.c, sg.c};
                v2f s0 = c * f.uy, l0 = __builtin_elementwise_fma(f.py, c, f.nt);  // one rounding each, as in the general form's chains
                if (!windowed) {
                    do scan_trip<true, ROWS_IN_LDS>(rows, spheres, off, end, a0, a1, f, s0, l0, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
                    while (off != end);
                } else {
                    for (;;) {
                        while (!need && (chunk + 64u) * kTripBytes < seg_end) {
                            chunk += 64u;
                            const uint32_t n = seg_end / kTripBytes - chunk;  // trips of the run from the chunk's first on: lanes below it test one each
                            bool mine = false;
                            if (lane < n) {
                                const ScanTripSpan sp = load_scan_span(sc, chunk + lane);
                                mine = scan_window_needs(sp.lo, sp.hi, x0, x1);
                            }
                            need = scan_window_fill(__ballot(mine));
                        }
                        if (!need) break;
                        const uint32_t first = (uint32_t)__builtin_ctzll(need);
                        const unsigned long long behind = ~(need >> first);  // bit 0 clear; no bit set: the range ends with the chunk
                        const uint32_t len = behind ? (uint32_t)__builtin_ctzll(behind) : 64u - first;
                        need &= need + (1ull << first);  // the lowest range of set bits leaves
                        const uint32_t start = (chunk + first) * kTripBytes;
                        if (start != off) {
                            off = start;
                            a0 = load_scan_pair(rows, off, 0u);
                            a1 = load_scan_pair(rows, off, kPairBytes);
                        }
                        end = start + len * kTripBytes;
#if RT_PHASES
                        ss.win_ranges++;
                        ss.win_trips += len;
#endif
                        do scan_trip<true, ROWS_IN_LDS>(rows, spheres, off, end, a0, a1, f, s0, l0, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
                        while (off != end);
                    }
                }
                if (off != seg_end) {  // the window ended short of the run: set A of what follows
                    off = seg_end;
                    a0 = load_scan_pair(rows, off, 0u);
                    a1 = load_scan_pair(rows, off, kPairBytes);
                }
                if (sg.axis == 0u) { scan_swap(f.ux, f.uy); scan_swap(f.px, f.py); }
                if (sg.axis == 2u) { scan_swap(f.uz, f.uy); scan_swap(f.pz, f.py); }
            }
        }
    }
    drain_filtered<ROWS_IN_LDS>(spheres, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
    if (best_k == kNone) return false;
    best.t = closest;
    best.ref = make_ref(REF_SPHERE, best_k);
    best.obj = kNone;
    return true;
}

// Pixel-parallel scan through the filter: sphere rows are wave-uniform (scalar path), eight per trip in two register sets
// as in scan_uniform below.
template <bool ROWS_IN_LDS>
DEV bool scan_filtered(const DeviceScene &sc, uint32_t planes_off, uint32_t n_padded, uint16_t *queue, uint32_t lane, const Ray &r, double tmin,
                       double tmax, HitInfo &best SS_ARG)
{
    const SphereScanRow *__restrict__ rows = sc.sphere_scan;
    const SphereGeom *__restrict__ spheres = sc.spheres;
    const uint32_t n = sc.n_spheres;
    const uint32_t n8 = n & ~7u;
    const double a = dot(r.d, r.d);
    const ScanRay f = scan_ray(r, a, sc.scan_reach);
    double closest = tmax;
    uint32_t best_k = kNone, count = 0;
    SphereScanRow a0{}, a1{}, a2{}, a3{};
    if (n8) {
        a0 = load_scan_row(rows, 0); a1 = load_scan_row(rows, 1);
        a2 = load_scan_row(rows, 2); a3 = load_scan_row(rows, 3);
    }
    for (uint32_t k0 = 0; k0 < n8; k0 += 8) {
        scan_rows_arrived(a0, a1, a2, a3);
        const SphereScanRow b0 = load_scan_row(rows, k0 + 4), b1 = load_scan_row(rows, k0 + 5);
        const SphereScanRow b2 = load_scan_row(rows, k0 + 6), b3 = load_scan_row(rows, k0 + 7);
        filter_four(a0, a1, a2, a3, k0, f, queue, lane, count);
        const uint32_t kn = (k0 + 8 < n8) ? k0 + 8 : k0;  // last trip re-reads its own rows (stays in bounds)
        scan_rows_arrived(b0, b1, b2, b3);
        a0 = load_scan_row(rows, kn); a1 = load_scan_row(rows, kn + 1);
        a2 = load_scan_row(rows, kn + 2); a3 = load_scan_row(rows, kn + 3);
        filter_four(b0, b1, b2, b3, k0 + 4, f, queue, lane, count);
        if (__any(count > (uint32_t)(kQueueCap - kFilterTrip))) drain_filtered<ROWS_IN_LDS>(spheres, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
    }
    for (uint32_t k = n8; k < n; k++) {
        const SphereScanRow g = load_scan_row(rows, k);
        const double s = filter_s(f, g.cx, g.cy, g.cz);
        const double q = filter_q(f, s, g.cx, g.cy, g.cz);
        if (q > g.k && !filter_behind(f, s, q, g.k)) {
            queue[count * 64u + lane] = (uint16_t)k;
            count++;
        }
        if (__any(count >= (uint32_t)kQueueCap)) drain_filtered<ROWS_IN_LDS>(spheres, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
    }
    drain_filtered<ROWS_IN_LDS>(spheres, planes_off, n_padded, queue, lane, count, r, a, tmin, closest, best_k SS_PASS);
    if (best_k == kNone) return false;
    best.t = closest;
    best.ref = make_ref(REF_SPHERE, best_k);
    best.obj = kNone;
    return true;
}

// Pixel-parallel scan: every live lane traces its own ray; sphere rows are wave-uniform (scalar path).
DEV bool scan_uniform(const DeviceScene &sc, uint16_t *queue, uint32_t lane, const Ray &r, double tmin, double tmax, HitInfo &best)
{
    const SphereGeom *__restrict__ spheres = sc.spheres;
    const uint32_t n = sc.n_spheres;
    const uint32_t n8 = n & ~7u;
    const double a = dot(r.d, r.d);
    double closest = tmax;
    uint32_t best_k = kNone, count = 0;
    // Eight rows per trip in two register sets (A, B): while one set is evaluated the other one's scalar loads are
    // in flight, and no set is ever copied into another.
    SphereGeom a0{}, a1{}, a2{}, a3{};
    if (n8) {
        a0 = load_sphere_row(spheres, 0); a1 = load_sphere_row(spheres, 1);
        a2 = load_sphere_row(spheres, 2); a3 = load_sphere_row(spheres, 3);
    }
    for (uint32_t k0 = 0; k0 < n8; k0 += 8) {
        rows_arrived(a0, a1, a2, a3);
        const SphereGeom b0 = load_sphere_row(spheres, k0 + 4), b1 = load_sphere_row(spheres, k0 + 5);
        const SphereGeom b2 = load_sphere_row(spheres, k0 + 6), b3 = load_sphere_row(spheres, k0 + 7);
        scan_four(a0, a1, a2, a3, k0, r, a, queue, lane, count);
        const uint32_t kn = (k0 + 8 < n8) ? k0 + 8 : k0;  // last trip re-reads its own rows (stays in bounds)
        rows_arrived(b0, b1, b2, b3);
        a0 = load_sphere_row(spheres, kn); a1 = load_sphere_row(spheres, kn + 1);
        a2 = load_sphere_row(spheres, kn + 2); a3 = load_sphere_row(spheres, kn + 3);
        scan_four(b0, b1, b2, b3, k0 + 4, r, a, queue, lane, count);
        if (__any(count > (uint32_t)(kQueueCap - 8))) drain_queue(spheres, queue, lane, count, r, a, tmin, closest, best_k);
    }
    for (uint32_t k = n8; k < n; k++) {
        scan_one(load_sphere_row(spheres, k), k, r, a, queue, lane, count);
        if (__any(count >= (uint32_t)kQueueCap)) drain_queue(spheres, queue, lane, count, r, a, tmin, closest, best_k);
    }
    drain_queue(spheres, queue, lane, count, r, a, tmin, closest, best_k);
    if (best_k == kNone) return false;
    best.t = closest;
    best.ref = make_ref(REF_SPHERE, best_k);
    best.obj = kNone;
    return true;
}

DEV double bcast(double x, int src_lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(x), src_lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(x), src_lane);
    return __hiloint2double(hi, lo);
}

// Sphere table as seen by the cooperative scan: four SoA planes in LDS (consecutive lanes read consecutive
// 8-byte words: conflict-free), or the global AoS table when it does not fit.
struct SphereView {
    // The LDS planes are addressed as byte offsets off the __shared__ symbol (plane(p, k)), never through pointers: a
    // pointer that may be LDS or global makes the compiler emit flat loads (19 of them in this kernel before), which are
    // slower than ds_read and tie up both wait counters.
    uint32_t planes_off;  // byte offset of plane 0 (cx); planes of n_padded doubles: cx, cy, cz, r2, K (filter_four's |c|^2 - r^2)
    double reach;         // DeviceScene::scan_reach
    bool exact;           // RT_FLAG_EXACT_SCAN: the reference's discriminant for every sphere, no filter
    const SphereGeom *global;
    uint32_t n, n_padded;
    bool in_lds;
    // The grouped scan's packed fp32 filter rows, two planes of 16 B a pair behind the fp64 planes: {cx0, cx1, cy0, cy1} of pair j at
    // pairs_off + 16 j, {cz0, cz1, k0, k1} at pairs_off + 16 (n_padded / 2 + j), in the general form (a run's rows swapped back).
    // Lane s of a group reads pair base + s with one ds_read_b128 per plane: the lanes of a group read consecutive 16-byte slots and
    // all groups the same ones.  Bank of a slot = 4 (slot mod 16) ... + 3; the instruction serves lanes {0-3, 12-15, 20-27},
    // {4-11, 16-19, 28-31} and the same two sets + 32 in one cycle each, and for every g = 2 ... 64 the slots such a set reads are
    // distinct mod 16 or equal (a broadcast): g >= 16 reads slots {0-3, 12-15, 4-11} (+16, +32, +48) of the batch, g = 8 slots
    // 0-7 twice, g = 4, 2, 1 fewer.  No bank conflicts.
    uint32_t pairs_off;   // 0: not staged, or RT_FLAG_FILTER_FP64 -- the grouped scan filters in fp64
    double reach32;       // DeviceScene::scan_reach32
    DEV double plane(uint32_t p, uint32_t k) const
    {
        return reinterpret_cast<const double *>(lds_raw + planes_off)[p * n_padded + k];
    }
};

// Wave-wide minimum of (t, k) pairs with DPP row operations (no LDS traffic); result valid in every lane.
// t > 0 always, so comparing (t, k) lexicographically picks the closest root, lowest sphere index on ties.
template <int CTRL, int ROW_MASK>
DEV void min_step(double &t, uint32_t &k)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(t), __double2loint(t), CTRL, ROW_MASK, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(t), __double2hiint(t), CTRL, ROW_MASK, 0xf, false);
    uint32_t ok = (uint32_t)__builtin_amdgcn_update_dpp((int)k, (int)k, CTRL, ROW_MASK, 0xf, false);
    double ot = __hiloint2double(hi, lo);
    bool take = (ot < t) || (ot == t && ok < k);
    t = take ? ot : t;
    k = take ? ok : k;
}
DEV void wave_min(double &t, uint32_t &k)
{
    min_step<0xB1, 0xf>(t, k);   // quad_perm [1,0,3,2]
    min_step<0x4E, 0xf>(t, k);   // quad_perm [2,3,0,1]
    min_step<0x114, 0xf>(t, k);  // row_shr:4
    min_step<0x118, 0xf>(t, k);  // row_shr:8   -> lane 15 of each row holds the row minimum
    min_step<0x142, 0xa>(t, k);  // row_bcast:15 into rows 1 and 3
    min_step<0x143, 0xc>(t, k);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave minimum
    t = bcast(t, 63);
    k = (uint32_t)__builtin_amdgcn_readlane((int)k, 63);
}

// Ray-cooperative scan: all 64 lanes work on ONE ray (lane `src`'s), lane l testing spheres l, l+64, ...;
// then a wave-wide min over (t, index).  Same winner as the sequential scan: that scan returns the smallest
// "first acceptable root" over all spheres with ties going to the lowest index, and a root that would have
// been rejected only because of an earlier closer hit loses the min here as well.
DEV void scan_cooperative(const SphereView &sv, uint32_t lane, unsigned long long todo, const Ray &ray, double tmin, double tmax,
                          HitInfo &best, bool &hit)
{
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        Ray r;
        r.o = mk(bcast(ray.o.x, src), bcast(ray.o.y, src), bcast(ray.o.z, src));
        r.d = mk(bcast(ray.d.x, src), bcast(ray.d.y, src), bcast(ray.d.z, src));
        const double a = dot(r.d, r.d);
        double bt = tmax;
        uint32_t bk = kNone;
        if (sv.in_lds && !sv.exact) {
            const ScanRay f = scan_ray(r, a, sv.reach);
            for (uint32_t base = 0; base < sv.n_padded; base += 256u) {
                double q[4];
                bool pass[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    uint32_t k = base + 64u * u + lane;
                    k = k < sv.n_padded ? k : sv.n_padded - 1u;
                    const double cx = sv.plane(0, k), cy = sv.plane(1, k), cz = sv.plane(2, k);
                    const double fs = filter_s(f, cx, cy, cz);
                    q[u] = filter_q(f, fs, cx, cy, cz);
                    pass[u] = q[u] > sv.plane(4, k);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t k = base + 64u * u + lane;
                    if (k < sv.n && pass[u]) {  // the reference's whole test for the survivors
                        double t;
                        if (sphere_test(r.o - mk(sv.plane(0, k), sv.plane(1, k), sv.plane(2, k)), r.d, a, sv.plane(3, k), tmin, bt, t)) {
                            bt = t;
                            bk = k;
                        }
                    }
                }
            }
        } else if (sv.in_lds) {
            for (uint32_t base = 0; base < sv.n_padded; base += 256u) {
                double b[4], c[4], disc[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    // rows past n_padded are never read: clamp keeps the address inside the planes
                    uint32_t k = base + 64u * u + lane;
                    k = k < sv.n_padded ? k : sv.n_padded - 1u;
                    Vec oc = r.o - mk(sv.plane(0, k), sv.plane(1, k), sv.plane(2, k));
                    b[u] = dot(oc, r.d);
                    c[u] = dot(oc, oc) - sv.plane(3, k);
                    disc[u] = b[u] * b[u] - a * c[u];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t k = base + 64u * u + lane;
                    if (k < sv.n && disc[u] > 0.0 && !(b[u] > 0.0 && c[u] > 0.0)) {
                        double t;
                        if (sphere_roots(b[u], disc[u], a, tmin, bt, t)) {
                            bt = t;
                            bk = k;
                        }
                    }
                }
            }
        } else {
            for (uint32_t k = lane; k < sv.n; k += 64u) {
                SphereGeom g = sv.global[k];
                Vec oc = r.o - mk(g.cx, g.cy, g.cz);
                double b = dot(oc, r.d);
                double c = dot(oc, oc) - g.r2;
                double disc = b * b - a * c;
                if (disc > 0.0 && !(b > 0.0 && c > 0.0)) {
                    double t;
                    if (sphere_roots(b, disc, a, tmin, bt, t)) {
                        bt = t;
                        bk = k;
                    }
                }
            }
        }
        wave_min(bt, bk);
        if ((int)lane == src) {
            hit = bk != kNone;
            best.t = bt;
            best.ref = make_ref(REF_SPHERE, bk);
            best.obj = kNone;
        }
    }
}

// Lane exchange through the LDS crossbar (ds_bpermute: no memory traffic).
DEV int lane_read(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }
DEV double lane_read(double x, int src_lane)
{
    int lo = lane_read(__double2loint(x), src_lane);
    int hi = lane_read(__double2hiint(x), src_lane);
    return __hiloint2double(hi, lo);
}
DEV void min_with_lane(double &t, uint32_t &k, int partner)
{
    double ot = lane_read(t, partner);
    uint32_t ok = (uint32_t)lane_read((int)k, partner);
    bool take = (ot < t) || (ot == t && ok < k);
    t = take ? ot : t;
    k = take ? ok : k;
}

// Ray-cooperative scan for a thin wave, several rays at a time: the L live rays are dealt to L groups of g = 64 / m
// lanes (m = L rounded up to a power of two), lane s of a group tests spheres s, s+g, s+2g, ...; one reduction over
// (t, index) per group serves all the rays at once.  Same winner as scan_cooperative (and as the sequential scan),
// at 1/L of its per-ray bookkeeping; against the pixel-parallel scan every lane does 1/g of the sphere tests.
//
// The packed fp32 branch queues its survivors (r36): a sphere that passes a lane's filter and is not behind goes to that lane's
// column of the survivor queue (idle in a grouped pass), as in filter_pairs / append_survivor, and the lanes run the reference's
// test on their own entries in ascending order against their running hit behind the last iteration -- drain_filtered itself: its
// signature fits, and it reads the rows from the fp64 planes as the tests in place did.  A lane meets its survivors in the order
// and with the running hit it met them in place, so its (t, index) is the same bit for bit, and the wave runs the test
// max-over-lanes-of-count times instead of once per slot that some lane passed (C2: 1.18 iterations a pass against 3.66 blocks).
// Queue bound, as above scan_filtered32: `count` changes only in append_survivor; at the head of an iteration every lane holds
// at most kQueueCap - 4 entries (true at the start, kept by an iteration that appends nothing, restored by the drain test behind
// every iteration in which some lane passed a sphere); an iteration appends at most its 4 spheres, so a lane writes its slot
// `count` only while count < kQueueCap.
DEV void scan_grouped(const SphereView &sv, uint16_t *queue, uint32_t lane, unsigned long long todo, const Ray &ray, double tmin, double tmax,
                      HitInfo &best, bool &hit GS_ARG)
{
    const int L = __popcll(todo);
    int log2m = 0;
    while ((1 << log2m) < L) log2m++;
    const int log2g = 6 - log2m;
    const uint32_t g = 1u << log2g;
    const uint32_t q = lane >> log2g, s = lane & (g - 1u);  // my ray slot and my place in its group
    // owner of slot q = the q-th live lane.  L rays go to m >= L groups: a group without a ray (q >= L) scans the FIRST ray once
    // more, in step with group 0 -- the same spheres pass in the same slots, so it adds no block, and nobody reads its result.
    // (Left with their own lanes' registers, each lane of such a group scanned another stale ray, and what the filters call
    // degenerate passes every sphere: on C2 109.7 of the 118.1 lanes tested per pass were theirs, profiles/r26_c2_grouped_far.txt.)
    int owner = todo ? __ffsll((long long)todo) - 1 : (int)lane;
    {
        unsigned long long m = todo;
        for (int r = 0; r < L; r++) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            owner = q == (uint32_t)r ? src : owner;
        }
    }
    Ray r;
    r.o = mk(lane_read(ray.o.x, owner), lane_read(ray.o.y, owner), lane_read(ray.o.z, owner));
    r.d = mk(lane_read(ray.d.x, owner), lane_read(ray.d.y, owner), lane_read(ray.d.z, owner));
    const double a = dot(r.d, r.d);
    double bt = tmax;
    uint32_t bk = kNone;
    if (!sv.exact && sv.pairs_off) {
        // The packed fp32 filter (filter_pairs' general form, operation for operation) over PAIRS: lane s of a group takes pairs s,
        // s + g, ... = spheres 2 s, 2 s + 1, 2 (s + g), ...: still ascending, each survivor tested against the hit of the one before.
        const ScanRayPairs f = scan_ray_pairs(scan_ray32(r, a, sv.reach32));
        const uint32_t n_pairs = sv.n_padded / 2u;
        const v4f *rows = reinterpret_cast<const v4f *>(lds_raw + sv.pairs_off);
        uint32_t count = 0;
#if RT_PHASES
        ScanSums ss{};
        uint32_t gs_mine = 0;
        gs.rays = (uint32_t)L;
        const unsigned long long gs_t0 = __builtin_readcyclecounter();
#endif
        for (uint32_t base = 0; base < n_pairs; base += 2u * g) {
            v2f fs[2], fq[2], fk[2];
            uint32_t jj[2];
            bool on[2];  // this lane has a pair in this half of the iteration
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t j = base + g * h + s;
                on[h] = j < n_pairs;
                jj[h] = on[h] ? j : n_pairs - 1u;  // keeps the address inside the rows
                const v4f lo = rows[jj[h]], hi = rows[n_pairs + jj[h]];
                const v2f cx = {lo.x, lo.y}, cy = {lo.z, lo.w}, cz = {hi.x, hi.y};
                fk[h] = v2f{hi.z, hi.w};
                fs[h] = __builtin_elementwise_fma(cz, f.uz, __builtin_elementwise_fma(cy, f.uy, cx * f.ux));
                fq[h] = __builtin_elementwise_fma(fs[h], fs[h], __builtin_elementwise_fma(f.pz, cz, __builtin_elementwise_fma(f.py, cy, __builtin_elementwise_fma(f.px, cx, f.nt))));
            }
            const float sv4[4] = {fs[0].x, fs[0].y, fs[1].x, fs[1].y}, qv4[4] = {fq[0].x, fq[0].y, fq[1].x, fq[1].y};
            const float kv4[4] = {fk[0].x, fk[0].y, fk[1].x, fk[1].y};
            // A row behind the list's last sphere never passes, so no test of its index is needed: its k is +inf, in the table's own
            // padding (scene_builder.cpp, where sphere_scan32 is filled: "padding: never passes"; flat_scene.h SphereScanPair) and in
            // the rows the kernel stages behind the table (render_kernel: "never passes").
            const bool p[4] = {on[0] && qv4[0] > kv4[0], on[0] && qv4[1] > kv4[1], on[1] && qv4[2] > kv4[2], on[1] && qv4[3] > kv4[3]};
            const unsigned long long m[4] = {__ballot(p[0]), __ballot(p[1]), __ballot(p[2]), __ballot(p[3])};  // the compares' own lane masks
            if (__builtin_expect((m[0] | m[1] | m[2] | m[3]) != 0, 0)) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (!m[u]) continue;  // wave-uniform: no lane passed this slot
                    const float bu = f.od - sv4[u];
                    const bool behind = bu > f.root_m && __builtin_fmaf(bu, bu, kv4[u] - qv4[u]) > 0.0f;  // k = -inf (always passes): never behind
#if RT_PHASES
                    gs.survivors += (uint32_t)__popcll(__ballot(p[u] && !behind));
                    gs_mine += p[u] && !behind ? 1u : 0u;
#endif
                    append_survivor(queue, lane, count, 2u * jj[u >> 1] + (uint32_t)(u & 1), p[u] && !behind);
                }
                if (__any(count > (uint32_t)(kQueueCap - 4))) drain_filtered<true>(sv.global, sv.planes_off, sv.n_padded, queue, lane, count, r, a, tmin, bt, bk SS_PASS);
            }
        }
        drain_filtered<true>(sv.global, sv.planes_off, sv.n_padded, queue, lane, count, r, a, tmin, bt, bk SS_PASS);
#if RT_PHASES
        asm volatile("" ::"v"(bt), "v"(bk));
        for (int off = 32; off > 0; off >>= 1) gs_mine = max(gs_mine, (uint32_t)__shfl_xor((int)gs_mine, off, 64));
        gs.lane_max = gs_mine;
        gs.drains = ss.drains;
        gs.tests = ss.drain_iters;
        gs.test_cycles = ss.drain_cycles;
        gs.filter_cycles = (uint32_t)(__builtin_readcyclecounter() - gs_t0) - ss.drain_cycles;
#endif
    } else if (!sv.exact) {
        const ScanRay f = scan_ray(r, a, sv.reach);
#if RT_PHASES
        uint32_t gs_mine = 0;
        gs.rays = (uint32_t)L;
#endif
        for (uint32_t base = 0; base < sv.n_padded; base += 4u * g) {
            bool pass[4];
#if RT_PHASES
            const unsigned long long gs_t0 = __builtin_readcyclecounter();
#endif
#pragma unroll
            for (int u = 0; u < 4; u++) {
                uint32_t k = base + g * u + s;
                k = k < sv.n_padded ? k : sv.n_padded - 1u;  // keeps the address inside the planes
                const double cx = sv.plane(0, k), cy = sv.plane(1, k), cz = sv.plane(2, k);
                const double fs = filter_s(f, cx, cy, cz);
                pass[u] = filter_q(f, fs, cx, cy, cz) > sv.plane(4, k);
            }
#if RT_PHASES
            const unsigned long long gs_t1 = __builtin_readcyclecounter();  // behind the compares: the ballots below read their masks
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const bool tested = base + g * u + s < sv.n && pass[u];
                const unsigned long long m = __ballot(tested);
                gs.tests += m ? 1u : 0u;
                gs.survivors += (uint32_t)__popcll(m);
                gs_mine += tested ? 1u : 0u;
            }
            const unsigned long long gs_t2 = __builtin_readcyclecounter();
            gs.filter_cycles += (uint32_t)(gs_t1 - gs_t0);
#endif
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t k = base + g * u + s;
                if (k < sv.n && pass[u]) {  // the reference's whole test for the survivors
                    double t;
                    if (sphere_test(r.o - mk(sv.plane(0, k), sv.plane(1, k), sv.plane(2, k)), r.d, a, sv.plane(3, k), tmin, bt, t)) {
                        bt = t;
                        bk = k;
                    }
                }
            }
#if RT_PHASES
            asm volatile("" ::"v"(bt), "v"(bk));
            gs.test_cycles += (uint32_t)(__builtin_readcyclecounter() - gs_t2);
#endif
        }
#if RT_PHASES
        for (int off = 32; off > 0; off >>= 1) gs_mine = max(gs_mine, (uint32_t)__shfl_xor((int)gs_mine, off, 64));
        gs.lane_max = gs_mine;
#endif
    } else
    for (uint32_t base = 0; base < sv.n_padded; base += 4u * g) {
        double b[4], c[4], disc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            uint32_t k = base + g * u + s;
            k = k < sv.n_padded ? k : sv.n_padded - 1u;  // keeps the address inside the planes
            Vec oc = r.o - mk(sv.plane(0, k), sv.plane(1, k), sv.plane(2, k));
            b[u] = dot(oc, r.d);
            c[u] = dot(oc, oc) - sv.plane(3, k);
            disc[u] = b[u] * b[u] - a * c[u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t k = base + g * u + s;
            if (k < sv.n && disc[u] > 0.0 && !(b[u] > 0.0 && c[u] > 0.0)) {
                double t;
                if (sphere_roots(b[u], disc[u], a, tmin, bt, t)) {
                    bt = t;
                    bk = k;
                }
            }
        }
    }
    // minimum over the group: partners at distance 1, 2 (quad permutes), 4 (half-row mirror), 8 (row mirror), then 16, 32
    if (log2g >= 1) min_step<0xB1, 0xf>(bt, bk);   // quad_perm [1,0,3,2]
    if (log2g >= 2) min_step<0x4E, 0xf>(bt, bk);   // quad_perm [2,3,0,1]
    if (log2g >= 3) min_step<0x141, 0xf>(bt, bk);  // row_half_mirror
    if (log2g >= 4) min_step<0x140, 0xf>(bt, bk);  // row_mirror
    if (log2g >= 5) min_with_lane(bt, bk, (int)lane ^ 16);
    if (log2g >= 6) min_with_lane(bt, bk, (int)lane ^ 32);
    // back to the owners: live lane number r reads the first lane of group r
    const int rank = __popcll(todo & ((1ull << lane) - 1ull));
    const double rt = lane_read(bt, rank << log2g);
    const uint32_t rk = (uint32_t)lane_read((int)bk, rank << log2g);
    if ((todo >> lane) & 1ull) {
        hit = rk != kNone;
        best.t = rt;
        best.ref = make_ref(REF_SPHERE, rk);
        best.obj = kNone;
    }
}

// ---- lanes-per-ray scan of a list world (R/HittableList.h:39-57) ---------------------------------------------------------
// A pixel's samples are one sequential chain (one RNG stream), so when a launch has fewer pixels than the device has lanes
// -- a small frame, one rank's stripes of a frame -- nothing shortens the frame but a shorter chain per ray.  With
// pixels_per_wave = 64 / g the pixels sit in the wave's first 64 / g lanes and the g lanes of group q share the ray of lane
// q: lane s of the group tests leaves s, s + g, ... with its own running closest hit, then one reduction per group picks
// the hit HittableList::Hit returns.  Which one that is when two leaves answer the SAME t depends on the kinds: a sphere
// is accepted for t < closest only (R/Sphere.h:38,50), a quad -- hence a box face, an instanced box -- for t <= closest
// (R/Quad.h:59-64 rejects t > tMax only).  Walking the list in order, the first leaf that reaches the final t sets it, a
// later quad at that t replaces it, a later sphere does not: the winner is the LAST quad among the tied leaves if there is
// one, else the FIRST sphere.  `key` orders exactly that (quads above spheres, later quads and earlier spheres higher),
// and every lane's own sub-sequence obeys the same rule by running the reference's tests in order.  A leaf's answer under
// a looser bound than the list would have given it is the same answer or one that loses the reduction (no leaf draws
// random numbers in these kernels: T::MEDIA is false), so the frame is the sequential scan's bit for bit.
template <int CTRL, int ROW_MASK>
DEV void tie_step(double &t, uint32_t &key)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(t), __double2loint(t), CTRL, ROW_MASK, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(t), __double2hiint(t), CTRL, ROW_MASK, 0xf, false);
    uint32_t ok = (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, CTRL, ROW_MASK, 0xf, false);
    double ot = __hiloint2double(hi, lo);
    bool take = (ot < t) || (ot == t && ok > key);
    t = take ? ot : t;
    key = take ? ok : key;
}
DEV void tie_with_lane(double &t, uint32_t &key, int partner)
{
    double ot = lane_read(t, partner);
    uint32_t ok = (uint32_t)lane_read((int)key, partner);
    bool take = (ot < t) || (ot == t && ok > key);
    t = take ? ot : t;
    key = take ? ok : key;
}

template <class T>
DEV bool leaf_test(const DeviceScene &sc, uint32_t ref, const Ray &r, double a, double tmin, double tmax, HitInfo &best, Xorwow &rng PH_ARG);

template <class T>
DEV void scan_leaves_grouped(const DeviceScene &sc, uint32_t lane, int log2g, unsigned long long todo, const Ray &ray, double tmin, double tmax,
                             HitInfo &best, bool &hit, Xorwow &rng PH_ARG)
{
    const uint32_t g = 1u << log2g;
    const uint32_t q = lane >> log2g, s = lane & (g - 1u);  // group q serves the pixel of lane q; my place in the group
    Ray r;
    r.o = mk(lane_read(ray.o.x, (int)q), lane_read(ray.o.y, (int)q), lane_read(ray.o.z, (int)q));
    r.d = mk(lane_read(ray.d.x, (int)q), lane_read(ray.d.y, (int)q), lane_read(ray.d.z, (int)q));
    r.tm = lane_read(ray.tm, (int)q);
    const bool wanted = ((todo >> q) & 1ull) != 0;
    const double a = dot(r.d, r.d);
    const uint32_t n = sc.n_world_items;
    HitInfo mine;
    mine.t = 0.0;
    mine.ref = kNone;
    mine.obj = kNone;
    double closest = tmax;
    uint32_t k_best = 0;
    bool any = false;
    if (wanted) {
        for (uint32_t k = s; k < n; k += g) {
            const uint32_t ref = ((const RT_CONST uint32_t *)(uintptr_t)sc.world_items)[k];
            if (leaf_test<T>(sc, ref, r, a, tmin, closest, mine, rng PH_PASS)) {
                any = true;
                closest = mine.t;
                k_best = k;
            }
        }
    }
    double wt = any ? closest : __builtin_inf();
    const uint32_t my_key = !any ? 0u : ((mine.ref >> kRefShift) == REF_QUAD ? (0x80000000u | k_best) : (0x7FFFFFFFu - k_best));
    uint32_t wkey = my_key;
    if (log2g >= 1) tie_step<0xB1, 0xf>(wt, wkey);   // quad_perm [1,0,3,2]
    if (log2g >= 2) tie_step<0x4E, 0xf>(wt, wkey);   // quad_perm [2,3,0,1]
    if (log2g >= 3) tie_step<0x141, 0xf>(wt, wkey);  // row_half_mirror
    if (log2g >= 4) tie_step<0x140, 0xf>(wt, wkey);  // row_mirror
    if (log2g >= 5) tie_with_lane(wt, wkey, (int)lane ^ 16);
    if (log2g >= 6) tie_with_lane(wt, wkey, (int)lane ^ 32);
    // every lane of a group now holds the group's (t, key); the lane whose own answer that is hands its record to the pixel's lane
    const unsigned long long holders = __ballot(any && my_key == wkey);
    const unsigned long long group_bits = log2g >= 6 ? holders : ((holders >> (lane << log2g)) & ((1ull << g) - 1ull));  // as owner: group `lane`
    const int src = (int)(lane << log2g) + (group_bits ? __ffsll((long long)group_bits) - 1 : 0);
    const double rt = lane_read(wt, src & 63);
    const uint32_t rref = (uint32_t)lane_read((int)mine.ref, src & 63);
    const uint32_t robj = (uint32_t)lane_read((int)mine.obj, src & 63);
    if (lane < (64u >> log2g) && ((todo >> lane) & 1ull)) {
        hit = group_bits != 0;
        best.t = rt;
        best.ref = rref;
        best.obj = robj;
    }
}

// The same grouped scan for a BVH world of spheres / unit-time moving spheres (config C3), for thin waves once the pixel
// queue has run dry.  A pixel's samples are one sequential chain, so a frame ends with a few long pixels (glass: up to
// max_depth rays per sample); walked, each of their rays costs ~36 dependent node visits with most of the wave idle.
// Scanned, the L live rays are dealt to groups of 64 / m lanes, every lane tests its share of ALL leaves (seven coalesced
// plane reads per row) and one reduction per group picks the hit -- the same hit as the walk's: no leaf draws random
// numbers, so the walk returns the closest acceptable root over all leaves (the reference's BVH = list invariant, Docs
// 2-3 BVH :733,:772), ties going to the lower leaf index here.  Centre and roots are computed exactly as prim_test does.
DEV void scan_grouped_ms(const DeviceScene &sc, uint32_t lane, unsigned long long todo, const Ray &ray, double tmin, double tmax,
                         HitInfo &best, bool &hit)
{
    const uint32_t n = sc.n_world_items, np = sc.ms_padded;
    const double *__restrict__ pl = sc.ms_planes;
    const int L = __popcll(todo);
    int log2m = 0;
    while ((1 << log2m) < L) log2m++;
    const int log2g = 6 - log2m;
    const uint32_t g = 1u << log2g;
    const uint32_t q = lane >> log2g, s = lane & (g - 1u);  // my ray slot and my place in its group
    int owner = (int)lane;
    {
        unsigned long long m = todo;
        for (int r = 0; r < L; r++) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            owner = q == (uint32_t)r ? src : owner;
        }
    }
    Ray r;
    r.o = mk(lane_read(ray.o.x, owner), lane_read(ray.o.y, owner), lane_read(ray.o.z, owner));
    r.d = mk(lane_read(ray.d.x, owner), lane_read(ray.d.y, owner), lane_read(ray.d.z, owner));
    r.tm = lane_read(ray.tm, owner);
    const double a = dot(r.d, r.d);
    double bt = tmax;
    uint32_t bk = kNone;
    for (uint32_t base = 0; base < np; base += 4u * g) {
        double b[4], c[4], disc[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            uint32_t k = base + g * u + s;
            k = k < np ? k : np - 1u;  // keeps the address inside the planes
            const Vec c0 = mk(pl[k], pl[np + k], pl[2u * np + k]);
            const Vec dc = mk(pl[3u * np + k], pl[4u * np + k], pl[5u * np + k]);
            const Vec centre = c0 + r.tm * dc;  // msphere_center with unit time (a static sphere: dc = 0)
            Vec oc = r.o - centre;
            b[u] = dot(oc, r.d);
            c[u] = dot(oc, oc) - pl[6u * np + k];
            disc[u] = b[u] * b[u] - a * c[u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t k = base + g * u + s;
            if (k < n && disc[u] > 0.0 && !(tmin >= 0.0 && b[u] > 0.0 && c[u] > 0.0)) {  // see sphere_test
                double t;
                if (sphere_roots(b[u], disc[u], a, tmin, bt, t)) {
                    bt = t;
                    bk = k;
                }
            }
        }
    }
    if (log2g >= 1) min_step<0xB1, 0xf>(bt, bk);   // quad_perm [1,0,3,2]
    if (log2g >= 2) min_step<0x4E, 0xf>(bt, bk);   // quad_perm [2,3,0,1]
    if (log2g >= 3) min_step<0x141, 0xf>(bt, bk);  // row_half_mirror
    if (log2g >= 4) min_step<0x140, 0xf>(bt, bk);  // row_mirror
    if (log2g >= 5) min_with_lane(bt, bk, (int)lane ^ 16);
    if (log2g >= 6) min_with_lane(bt, bk, (int)lane ^ 32);
    const int rank = __popcll(todo & ((1ull << lane) - 1ull));
    const double rt = lane_read(bt, rank << log2g);
    const uint32_t rk = (uint32_t)lane_read((int)bk, rank << log2g);
    if ((todo >> lane) & 1ull) {
        hit = rk != kNone;
        best.t = rt;
        best.ref = hit ? sc.world_items[rk] : kNone;
        best.obj = kNone;
    }
}

// ------------------------------------------------------------------------------------------------
// hit record, built once per bounce from (t, primitive)
// ------------------------------------------------------------------------------------------------
DEV void sphere_uv(Vec on, double &u, double &v)  // R/Sphere.h:74-81
{
    const double pi = 3.1415926535897932385;
    double theta = acos(-on.y);
    double phi = atan2(-on.z, on.x) + pi;
    u = phi / (2.0 * pi);
    v = theta / pi;
}

DEV void face(Surface &s, const Ray &r, Vec outward)  // R/Hittable.h:26-30
{
    s.front = dot(r.d, outward) < 0.0;
    s.n = s.front ? outward : -outward;
}

// Corner normals and texture coordinates of a triangle (include/rtow.h rt_triangle_attr has the operations, flat_scene.h TriAttrRow
// the row: quads[AAQuad::pad], behind the quad rows).  Scenes without such a triangle pay the scalar test of the scene flag per
// planar hit; the search never comes here.  attr_row: the row's index in quads[], 0 for a row without attributes.
DEV uint32_t attr_row(const DeviceScene &sc, uint32_t idx) { return (sc.flags & SCENE_VERTEX_ATTR) ? get_quad_aa(sc, idx).pad : 0u; }
DEV void attr_uv(const RT_CONST double *a, double alpha, double beta, double gamma, double &u, double &v)
{
    u = (gamma * a[9] + alpha * a[11]) + beta * a[13];
    v = (gamma * a[10] + alpha * a[12]) + beta * a[14];
}
// s.p: the hit point in the space the hit was found in; s.n, s.front: face()'s, of the geometric normal q.n
DEV void vertex_attr(const DeviceScene &sc, uint32_t row, const QuadGeom &q, bool want_uv, Surface &s)
{
    const RT_CONST double *a = const_doubles(sc.quads + row);
    const uint32_t kinds = ((const RT_CONST uint32_t *)a)[30];
    const Vec ph = s.p - mk(q.qx, q.qy, q.qz), w = mk(q.wx, q.wy, q.wz);
    const double alpha = dot(w, cross(ph, mk(q.vx, q.vy, q.vz)));
    const double beta = dot(w, cross(mk(q.ux, q.uy, q.uz), ph));
    const double gamma = (1.0 - alpha) - beta;
    if (kinds & ATTR_NORMALS) {
        const Vec ng = mk(q.nx, q.ny, q.nz);
        const Vec m = (gamma * mk(a[0], a[1], a[2]) + alpha * mk(a[3], a[4], a[5])) + beta * mk(a[6], a[7], a[8]);
        const double lsq = length_sq(m);
        Vec ns = unit(m);
        if (!(lsq > 0.0 && lsq < (double)INFINITY) || dot(ns, ng) <= 0.0) ns = ng;  // never under the geometric surface
        s.n = s.front ? ns : -ns;
    }
    if (want_uv && (kinds & ATTR_TEXCOORDS)) attr_uv(a, alpha, beta, gamma, s.u, s.v);
}

template <class T>
DEV Surface make_surface(const DeviceScene &sc, const Ray &r, const HitInfo &h)
{
    Surface s;
    s.u = 0.0;
    s.v = 0.0;
    uint32_t tag = h.ref >> kRefShift, idx = h.ref & kRefIndexMask;
    // the transforms between the world and the space the hit was found in (outermost first), if any
    uint32_t xf_first = 0, xf_count = 0;
    Ray lr = r;
    if constexpr (T::COMPOSITE) {
        if (h.obj != kNone) {
            if (T::NESTED && (h.obj & kTreeObjBit)) {  // inside a tree: the winning node's chain
                const TreeNodeRec n = sc.tree_nodes[h.obj & ~kTreeObjBit];
                xf_first = n.chain_first;
                xf_count = n.chain_count;
            } else if (tag != REF_MEDIUM) {
                const ObjectRec o = get_object(sc, h.obj);
                xf_first = o.xf_first;
                xf_count = o.xf_count;
            }
            lr = chain_ray(sc, xf_first, xf_count, r);
        }
    }
    bool is_medium = false;
    if constexpr (T::MEDIA) is_medium = tag == REF_MEDIUM;
    if (is_medium) {  // R/ConstantMedium.h:86-91
        s.p = at(lr, h.t);
        s.n = mk(1, 0, 0);
        s.front = true;
        s.mat = get_medium(sc, idx).phase_mat;
    } else
    if (T::WORLD != 2 && tag == REF_QUAD) {  // R/Quad.h:86-96
        s.p = at(lr, h.t);
        QuadGeom q = sc.quads[idx];
        s.mat = sc.quad_mat[idx];
        face(s, lr, mk(q.nx, q.ny, q.nz));
        if constexpr (T::RICH) {
            if (material_needs_uv(sc, s.mat)) {
                Vec ph = s.p - mk(q.qx, q.qy, q.qz);
                Vec w = mk(q.wx, q.wy, q.wz);
                s.u = dot(w, cross(ph, mk(q.vx, q.vy, q.vz)));
                s.v = dot(w, cross(mk(q.ux, q.uy, q.uz), ph));
            }
        }
        if (const uint32_t row = attr_row(sc, idx)) {
            bool want_uv = false;
            if constexpr (T::RICH) want_uv = material_needs_uv(sc, s.mat);
            vertex_attr(sc, row, q, want_uv, s);
        }
    } else {  // R/Sphere.h:40-46
        s.p = at(lr, h.t);
        Vec c;
        SphereAux aux;
        if (T::WORLD == 2 || tag == REF_SPHERE) {
            SphereGeom g = T::COMPOSITE ? get_sphere(sc, idx) : (T::FAST ? get_sphere_typed(sc, idx) : sc.spheres[idx]);
            c = mk(g.cx, g.cy, g.cz);
            aux = T::FAST ? get_sphere_aux(sc, idx) : sc.sphere_aux[idx];
        } else {
            c = msphere_center(T::FAST ? get_msphere(sc, idx) : sc.mspheres[idx], lr.tm, (sc.flags & SCENE_MS_UNIT_TIME) != 0);
            aux = T::FAST ? get_msphere_aux(sc, idx) : sc.msphere_aux[idx];
        }
        Vec on = aux.inv_r * (s.p - c);
        face(s, lr, on);
        s.mat = aux.mat;
        if constexpr (T::RICH) {
            if (material_needs_uv(sc, s.mat)) sphere_uv(on, s.u, s.v);
        }
    }
    if constexpr (T::COMPOSITE) {
        if (h.obj != kNone) {  // back to world space, innermost transform first (R/Instance.h:53,137-147)
            for (uint32_t k = xf_count; k-- > 0;) {
                Xform x = get_xform(sc, xf_first + k);
                if (x.kind == XF_TRANSLATE) {
                    s.p = s.p + mk(x.a, x.b, x.c);
                } else if (!kAffineUnit || x.kind == XF_ROTATE_Y) {
                    double st = x.a, ct = x.b;
                    s.p = mk((ct * s.p.x) + (st * s.p.z), s.p.y, (-st * s.p.x) + (ct * s.p.z));
                    s.n = mk((ct * s.n.x) + (st * s.n.z), s.n.y, (-st * s.n.x) + (ct * s.n.z));
                } else if (!kMovingUnit || __builtin_expect(x.pad == kAffineRows - 1, 1)) {  // x is the last row of the step
                    k -= kAffineRows - 1;
                    affine_to_world(sc, xf_first + k, s.p, s.n);
                } else {  // the last row of a moving step
                    k -= kMovingRows - 1;
                    moving_to_world(sc, xf_first + k, r.tm, s.p, s.n);
                }
            }
        }
    }
    return s;
}

// ------------------------------------------------------------------------------------------------
// textures and materials
// ------------------------------------------------------------------------------------------------
// perlin_noise (table in global memory) and perlin_noise_lds (table staged in LDS) are two codings of one sum, and which
// of them a launch runs is lds_layout's choice -- which must not show in the frame.  One is a rolled loop over the corners
// with run-time a, b, c, the other is unrolled with constants, and the fast build fused the multiply-adds of the two
// differently (two Perlin tables staged against three in global memory: 0.3 % of a marble frame's pixels differed).  So no
// product of either is fused into the add that follows it: it goes through unfused(), an empty asm that the backend cannot
// look through (the fast objects fuse in the backend whatever a contraction pragma says: adaptive_rule.h).  The strict build
// fuses nothing anyway and compiles exactly what it compiled without.
DEV double unfused(double x)
{
#if !RT_STRICT
    asm("" : "+v"(x));
#endif
    return x;
}
DEV double perlin_fade(double u) { return u * u * (3.0 - unfused(2.0 * u)); }
// the term of corner (a, b, c): its trilinear weight times gradient . offset, R/Perlin.h:120-139
DEV double perlin_corner(int a, int b, int c, double u, double v, double w, double uu, double vv, double ww, Vec g)
{
    const Vec wv = mk(u - a, v - b, w - c);
    const double wa = unfused(a * uu) + unfused((1 - a) * (1 - uu)), wb = unfused(b * vv) + unfused((1 - b) * (1 - vv));
    const double wc = unfused(c * ww) + unfused((1 - c) * (1 - ww));
    return unfused(wa * wb * wc * (unfused(g.x * wv.x) + unfused(g.y * wv.y) + unfused(g.z * wv.z)));
}
DEV double perlin_noise(const PerlinRec *pn, Vec p)  // R/Perlin.h:38-60,120-139
{
    double fx = floor(p.x), fy = floor(p.y), fz = floor(p.z);
    double u = p.x - fx, v = p.y - fy, w = p.z - fz;
    int i = (int)fx, j = (int)fy, k = (int)fz;
    double uu = perlin_fade(u), vv = perlin_fade(v), ww = perlin_fade(w);
    double accum = 0.0;
    // corners one after another (same summation order as the reference; keeps the register footprint small)
#pragma unroll 1
    for (int a = 0; a < 2; a++)
#pragma unroll 1
        for (int b = 0; b < 2; b++)
#pragma unroll 1
            for (int c = 0; c < 2; c++) {
                int idx = pn->perm_x[(i + a) & 255] ^ pn->perm_y[(j + b) & 255] ^ pn->perm_z[(k + c) & 255];
                Vec g = mk(pn->vec[idx][0], pn->vec[idx][1], pn->vec[idx][2]);
                accum += perlin_corner(a, b, c, u, v, w, uu, vv, ww, g);
            }
    return accum;
}

// The same from a table staged in LDS (layout of PerlinRec at byte offset `off`).  The global version above walks the
// eight corners one dependent load chain after another (56 chains of two L2 round trips per marble lookup: one marble
// lane held its whole wave for ~50k cycles); here the six permutation entries and the eight gradient rows are
// independent LDS reads, summed in the reference's corner order.
DEV double perlin_noise_lds(uint32_t off, Vec p)  // R/Perlin.h:38-60,120-139
{
    const double *vec = reinterpret_cast<const double *>(lds_raw + off);
    const int32_t *perm = reinterpret_cast<const int32_t *>(lds_raw + off + 256u * 3u * (uint32_t)sizeof(double));
    double fx = floor(p.x), fy = floor(p.y), fz = floor(p.z);
    double u = p.x - fx, v = p.y - fy, w = p.z - fz;
    int i = (int)fx, j = (int)fy, k = (int)fz;
    double uu = perlin_fade(u), vv = perlin_fade(v), ww = perlin_fade(w);
    const int px[2] = {perm[i & 255], perm[(i + 1) & 255]};
    const int py[2] = {perm[256 + (j & 255)], perm[256 + ((j + 1) & 255)]};
    const int pz[2] = {perm[512 + (k & 255)], perm[512 + ((k + 1) & 255)]};
    double accum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const int idx = px[a] ^ py[b] ^ pz[c];
                Vec g = mk(vec[idx * 3 + 0], vec[idx * 3 + 1], vec[idx * 3 + 2]);
                accum += perlin_corner(a, b, c, u, v, w, uu, vv, ww, g);
            }
    return accum;
}

DEV double perlin_turb(const DeviceScene &sc, uint32_t table, Vec p, int depth)  // R/Perlin.h:63-78
{
    double accum = 0.0, weight = 1.0;
    const bool in_lds = sc.lds_perlin != kNone;
    for (int i = 0; i < depth; i++) {
        accum += weight * (in_lds ? perlin_noise_lds(sc.lds_perlin + table * (uint32_t)sizeof(PerlinRec), p) : perlin_noise(sc.perlin + table, p));
        weight *= 0.5;
        p = 2.0 * p;
    }
    return fabs(accum);
}

template <class T>
DEV Vec texture_value(const DeviceScene &sc, uint32_t ti, double u, double v, Vec p)
{
    TextureRec t = sc.textures[ti];
    while (t.kind == TEX_CHECKER) {  // R/Texture.h:70-81
        int xi = (int)floor(t.s * p.x), yi = (int)floor(t.s * p.y), zi = (int)floor(t.s * p.z);
        bool even = ((xi + yi + zi) % 2) == 0;
        t = sc.textures[even ? t.a : t.b_];
    }
    if constexpr (T::RICH) {
        if (t.kind == TEX_IMAGE) {  // R/Texture.h:110-133
            ImageRec im = sc.images[t.a];
            if (im.height <= 0) return mk(0.0, 1.0, 1.0);
            u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
            v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
            v = 1.0 - v;
            int i = (int)(u * im.width), j = (int)(v * im.height);
            if (i >= im.width) i = im.width - 1;
            if (j >= im.height) j = im.height - 1;
            const unsigned char *px = sc.image_bytes + im.offset + ((size_t)j * im.width + i) * 3;
            double cs = 1.0 / 255.0;
            return mk(cs * px[0], cs * px[1], cs * px[2]);
        }
        if (t.kind == TEX_NOISE) {  // R/Texture.h:159-165: marble
            double sv = 1.0 + sin(t.s * p.z + 10.0 * perlin_turb(sc, t.a, p, 7));
            return sv * mk(0.5, 0.5, 0.5);
        }
    }
    return mk(t.r, t.g, t.b);  // TEX_SOLID, R/Texture.h:48-51
}

// One material row, read field by field from wherever the table lives: the LDS copy (small tables, launcher's choice)
// or the global table.  Which one is wave-uniform, so each read is one scalar branch and one load.
struct MatView {
    const MaterialRec *global;
    uint32_t lds_off;  // byte offset of the row in LDS, or kNone
    // The LDS side is read through a pointer typed for the LDS address space: two loads through generic pointers get merged
    // into one flat load through a selected pointer (slower than ds_read, and it ties up both wait counters).
    DEV double f64(uint32_t off) const
    {
        if (lds_off != kNone) return *(const RT_LDS double *)(lds_raw + lds_off + off);
        return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(global) + off);
    }
    DEV uint32_t u32(uint32_t off) const
    {
        if (lds_off != kNone) return *(const RT_LDS uint32_t *)(lds_raw + lds_off + off);
        return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(global) + off);
    }
    DEV Vec vec(uint32_t off) const { return mk(f64(off), f64(off + 8u), f64(off + 16u)); }
};
#define MAT_OFF(field) ((uint32_t)offsetof(MaterialRec, field))
// MAY_BE_STAGED = false (kernels that never stage materials): the LDS side folds away at compile time -- left in, the
// compiler merges the two loads of every field into one flat load through a selected pointer
template <bool MAY_BE_STAGED>
DEV MatView material_view(const DeviceScene &sc, uint32_t i)
{
    if constexpr (!MAY_BE_STAGED) return MatView{sc.materials + i, kNone};
    return MatView{sc.materials + i, sc.lds_materials != kNone ? sc.lds_materials + i * (uint32_t)sizeof(MaterialRec) : kNone};
}

// Texture of a material: host-resolved solid / checker-of-solids without touching the texture table.
template <class T>
DEV Vec material_texture(const DeviceScene &sc, const MatView &m, uint32_t tex_inline, double u, double v, Vec p)
{
    if (tex_inline == 1) return m.vec(MAT_OFF(even));
    if (tex_inline == 2) {  // R/Texture.h:70-81
        const double inv_scale = m.f64(MAT_OFF(inv_scale));
        int xi = (int)floor(inv_scale * p.x), yi = (int)floor(inv_scale * p.y), zi = (int)floor(inv_scale * p.z);
        bool even = ((xi + yi + zi) % 2) == 0;
        return m.vec(even ? MAT_OFF(even) : MAT_OFF(odd));
    }
    if constexpr (T::RICH) return texture_value<T>(sc, m.u32(MAT_OFF(tex)), u, v, p);
    return mk(0.0, 0.0, 0.0);  // unreachable: scenes with table-walking textures run the RICH instantiation
}

// pow(x, 5.0) of Schlick's approximation (R/Dielectric.h:61-67) by repeated multiplication: within 1.5 ulp of the
// correctly rounded value, i.e. the same accuracy class as any libm's pow (the reference's is CUDA's, the oracle's
// is glibc's, neither is bit-reproducible here).  The value only feeds the comparison `reflectance > uniform`.
// The library pow() costs ~45 VGPRs of kernel-wide register budget -- a whole wave per SIMD of occupancy.
DEV double pow5(double x)
{
    double x2 = x * x;
    double x4 = x2 * x2;
    return x4 * x;
}

DEV Vec random_in_unit_sphere(Xorwow &rng)  // R/Material.h:14-24
{
    Vec p;
    do {
        double a = (double)xorwow_uniform(rng);
        double b = (double)xorwow_uniform(rng);
        double c = (double)xorwow_uniform(rng);
        p = 2.0 * mk(a, b, c) - mk(1.0, 1.0, 1.0);
    } while (length_sq(p) >= 1.0);
    return p;
}

// Emitted + Scatter (R/kernel.cu:82-94).  Returns false when the path ends here.
// The in-sphere sample (Lambertian, Metal, Isotropic) and the unit direction (Metal, Dielectric) are evaluated
// once, ahead of the material switch, for the lanes whose material uses them: in each of those Scatter
// functions the sample is the first thing drawn from the RNG, so the per-pixel draw order is unchanged.
template <class T>
DEV bool shade(const DeviceScene &sc, const Surface &s, Ray &ray, Vec &throughput, Vec &accumulated, Xorwow &rng)
{
    // only the fields a material kind needs are loaded (the row is 112 bytes)
    const MatView mp = material_view<(T::COMPOSITE && T::WORLD == 0) || T::FAST>(sc, s.mat);
    struct { uint32_t kind, tex_inline; } m = {mp.u32(MAT_OFF(kind)), mp.u32(MAT_OFF(tex_inline))};
    Vec atten;
    Ray out;
    out.o = s.p;
    out.tm = ray.tm;
    Vec rs = mk(0.0, 0.0, 0.0), ud = mk(0.0, 0.0, 0.0);
    if (m.kind == MAT_LAMBERTIAN || m.kind == MAT_METAL || m.kind == MAT_ISOTROPIC) rs = random_in_unit_sphere(rng);
    if (m.kind == MAT_METAL || m.kind == MAT_DIELECTRIC) ud = unit(ray.d);
    switch (m.kind) {
    case MAT_DIFFUSE_LIGHT:  // R/Material.h:114-127: emits on both sides, never scatters
        accumulated = accumulated + throughput * material_texture<T>(sc, mp, m.tex_inline, s.u, s.v, s.p);
        return false;
    case MAT_LAMBERTIAN: {  // R/Material.h:67-82
        Vec dir = s.n + rs;
        if (fabs(dir.x) < 1e-8 && fabs(dir.y) < 1e-8 && fabs(dir.z) < 1e-8) dir = s.n;
        out.d = dir;
        atten = material_texture<T>(sc, mp, m.tex_inline, s.u, s.v, s.p);
        break;
    }
    case MAT_METAL: {  // R/Metal.h:18-30
        Vec refl = reflect(ud, s.n);
        out.d = refl + mp.f64(MAT_OFF(p)) * rs;
        atten = mp.vec(MAT_OFF(r));
        if (!(dot(out.d, s.n) > 0.0)) return false;
        break;
    }
    case MAT_DIELECTRIC: {  // R/Dielectric.h:18-68
        atten = mk(1.0, 1.0, 1.0);
        const double ior = mp.f64(MAT_OFF(p));
        double ratio = s.front ? (1.0 / ior) : ior;
        double ct = fmin(dot(-ud, s.n), 1.0);
        double st = sqrt(1.0 - ct * ct);
        bool reflect_it = ratio * st > 1.0;
        if (!reflect_it) {
            double r0 = (1.0 - ratio) / (1.0 + ratio);
            r0 = r0 * r0;
            double refl = r0 + (1.0 - r0) * pow5(1.0 - ct);
            reflect_it = refl > (double)xorwow_uniform(rng);
        }
        out.d = reflect_it ? reflect(ud, s.n) : refract(ud, s.n, ratio);
        break;
    }
    default: {  // MAT_ISOTROPIC, R/Material.h:152-163
        out.d = unit(rs);
        atten = material_texture<T>(sc, mp, m.tex_inline, s.u, s.v, s.p);
        break;
    }
    }
    throughput = throughput * atten;
    ray = out;
    return true;
}

// Camera::GetRay (R/Camera.h:76-85) behind the pixel jitter of Render (R/kernel.cu:140-142).
DEV Vec load3c(const RT_CONST double *p) { return mk(p[0], p[1], p[2]); }

// The environment (include/rtow.h rt_scene_set_environment states every operation; tests/environment_restated.py restates the
// strict build): the record behind the camera's (flat_scene.h EnvRec), valid only under SCENE_ENVIRONMENT.
DEV const RT_CONST EnvRec *environment_of(const CameraRec *cam) { return (const RT_CONST EnvRec *)(uintptr_t)(cam + 1); }
// the direction d, not necessarily unit, in the environment's frame, and its (u, v): the reference's GetSphereUV (R/Sphere.h:74-81)
DEV void environment_coords(const RT_CONST EnvRec *env, Vec d, Vec &e, double &u, double &v)
{
    const Vec n = (1 / sqrt((d.x * d.x + d.y * d.y) + d.z * d.z)) * d;
    e = mk((env->rot[0] * n.x + env->rot[1] * n.y) + env->rot[2] * n.z, (env->rot[3] * n.x + env->rot[4] * n.y) + env->rot[5] * n.z,
           (env->rot[6] * n.x + env->rot[7] * n.y) + env->rot[8] * n.z);
    sphere_uv(e, u, v);
}
// ImageTexture::Value's index rule (R/Texture.h:110-133) for a table of width x height texels, top row first; the index is
// clamped on both sides, so that no (u, v), a NaN included, names a texel outside the table
DEV void environment_texel(int width, int height, double u, double v, int &i, int &j)
{
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    v = 1.0 - v;
    i = (int)(u * width);
    j = (int)(v * height);
    i = i >= width ? width - 1 : (i < 0 ? 0 : i);
    j = j >= height ? height - 1 : (j < 0 ? 0 : j);
}
// the value at e, (u, v): intensity * the texture there, or intensity * the float image's texel widened to double
template <class T>
DEV Vec environment_lookup(const DeviceScene &sc, const RT_CONST EnvRec *env, Vec e, double u, double v)
{
    Vec value;
    if (env->texture != kNone) {
        value = texture_value<T>(sc, env->texture, u, v, e);
    } else {
        int i, j;
        environment_texel(env->width, env->height, u, v, i, j);
        const float *px = env->rgb + ((size_t)j * (size_t)env->width + (size_t)i) * 3;
        value = mk((double)px[0], (double)px[1], (double)px[2]);
    }
    return load3c(env->intensity) * value;
}
template <class T>
DEV Vec environment_value(const DeviceScene &sc, const CameraRec *cam, Vec d)
{
    const RT_CONST EnvRec *env = environment_of(cam);
    Vec e;
    double u, v;
    environment_coords(env, d, e, u, v);
    return environment_lookup<T>(sc, env, e, u, v);
}
// What a ray that leaves the world adds (R/kernel.cu:74-79): the environment along it where the scene has one -- one wave-uniform
// test of the scene's flags, compiled only into the instantiations that carry the texture code -- else the camera's background.
template <class T>
DEV Vec miss_value(const DeviceScene &sc, const CameraRec *cam, Vec d)
{
    if constexpr (T::RICH) {
        if ((sc.flags & SCENE_ENVIRONMENT) != 0) return environment_value<T>(sc, cam, d);
    }
    return load3c(((const RT_CONST CameraRec *)(uintptr_t)cam)->bg);
}

DEV Ray camera_ray(const CameraRec *cam_generic, int i, int j, int width, int height, Xorwow &rng)
{
    const RT_CONST CameraRec *cam = (const RT_CONST CameraRec *)(uintptr_t)cam_generic;
    double u = (double)((float)i + xorwow_uniform(rng)) / (double)width;   // int + float adds in fp32
    double v = (double)((float)j + xorwow_uniform(rng)) / (double)height;
    Vec p;
    do {
        double a = (double)xorwow_uniform(rng);
        double b = (double)xorwow_uniform(rng);
        p = 2.0 * mk(a, b, 0.0) - mk(1.0, 1.0, 0.0);
    } while (dot(p, p) >= 1.0);
    Vec rd = cam->lens_radius * p;
    Vec cu = load3c(cam->u), cv = load3c(cam->v);
    Vec offset = rd.x * cu + rd.y * cv;
    double tm = cam->time0 + (double)xorwow_uniform(rng) * (cam->time1 - cam->time0);
    Vec origin = load3c(cam->origin);
    Ray r;
    r.o = origin + offset;
    r.d = load3c(cam->llc) + u * load3c(cam->horizontal) + v * load3c(cam->vertical) - origin - offset;
    r.tm = tm;
    return r;
}

// Row of the full frame that local row `lr` of this rank maps to (stripes dealt round-robin).
DEV int owned_row(int lr, int stripe, int rank, int world)
{
    return ((lr / stripe) * world + rank) * stripe + (lr % stripe);
}

} // namespace
#if RT_AFFINE
}  // inline namespace affine
#endif

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
template <int STRICT>
__global__ __launch_bounds__(256) void seed_kernel(SeedArgs a)
{
    uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= a.n_pixels) return;
    int lr = (int)(local / (uint32_t)a.width), i = (int)(local % (uint32_t)a.width);
    int j = owned_row(lr, a.stripe_rows, a.rank, a.world_size);
    uint64_t sequence = (uint64_t)((int64_t)j * a.width + i);  // pixelIndex, R/kernel.cu:117-118
    Xorwow s = a.base;
    xorwow_skip_sequences(a.jump_table, sequence, s);
    a.state[0 * (size_t)a.n_pixels + local] = s.d;
    a.state[1 * (size_t)a.n_pixels + local] = s.v0;
    a.state[2 * (size_t)a.n_pixels + local] = s.v1;
    a.state[3 * (size_t)a.n_pixels + local] = s.v2;
    a.state[4 * (size_t)a.n_pixels + local] = s.v3;
    a.state[5 * (size_t)a.n_pixels + local] = s.v4;
}


#if RT_PHASES
DEV void ph_flush(const RenderArgs &a, PhaseSums &ph, unsigned long long ph_start, uint32_t lane)
{
    for (int k = 4; k < 15; k++) {
        if (k == 12 || k == 13) continue;  // wave-level slots
        for (int off = 32; off > 0; off >>= 1) {
            ph.t[k] += __shfl_down(ph.t[k], off, 64);
            ph.l[k] += __shfl_down(ph.l[k], off, 64);
            ph.n[k] += __shfl_down(ph.n[k], off, 64);
        }
        ph.t[k] >>= 10;
        ph.l[k] >>= 10;
        ph.n[k] >>= 10;
    }
    if (lane == 0) {
        for (int k = 0; k < 24; k++) {
            atomicAdd(a.ray_counter + 32 + k, ph.t[k]);
            atomicAdd(a.ray_counter + 64 + k, ph.l[k]);
            atomicAdd(a.ray_counter + 96 + k, ph.n[k]);
        }
        atomicAdd(a.ray_counter + 7, __builtin_readcyclecounter() - ph_start);
    }
}
#endif
// Parked path state (Traits::PARK): twelve 8-byte planes of BLOCK entries behind the staged tables, one entry per thread.
template <int BLOCK>
DEV void park_put(uint32_t off, int k, double v) { *(RT_LDS double *)(lds_raw + off + ((uint32_t)k * (uint32_t)BLOCK + threadIdx.x) * 8u) = v; }
template <int BLOCK>
DEV double park_get(uint32_t off, int k) { return *(const RT_LDS double *)(lds_raw + off + ((uint32_t)k * (uint32_t)BLOCK + threadIdx.x) * 8u); }
template <int BLOCK>
DEV void park_put_vec(uint32_t off, int k, Vec v) { park_put<BLOCK>(off, k, v.x); park_put<BLOCK>(off, k + 1, v.y); park_put<BLOCK>(off, k + 2, v.z); }
template <int BLOCK>
DEV Vec park_get_vec(uint32_t off, int k) { return mk(park_get<BLOCK>(off, k), park_get<BLOCK>(off, k + 1), park_get<BLOCK>(off, k + 2)); }
template <int BLOCK>
DEV void park_put_rng(uint32_t off, const Xorwow &g)
{
    RT_LDS uint32_t *p = (RT_LDS uint32_t *)(lds_raw + off + (9u * (uint32_t)BLOCK) * 8u);
    p[0 * BLOCK + threadIdx.x] = g.d;  p[1 * BLOCK + threadIdx.x] = g.v0; p[2 * BLOCK + threadIdx.x] = g.v1;
    p[3 * BLOCK + threadIdx.x] = g.v2; p[4 * BLOCK + threadIdx.x] = g.v3; p[5 * BLOCK + threadIdx.x] = g.v4;
}
template <int BLOCK>
DEV void park_get_rng(uint32_t off, Xorwow &g)
{
    const RT_LDS uint32_t *p = (const RT_LDS uint32_t *)(lds_raw + off + (9u * (uint32_t)BLOCK) * 8u);
    g.d = p[0 * BLOCK + threadIdx.x];  g.v0 = p[1 * BLOCK + threadIdx.x]; g.v1 = p[2 * BLOCK + threadIdx.x];
    g.v2 = p[3 * BLOCK + threadIdx.x]; g.v3 = p[4 * BLOCK + threadIdx.x]; g.v4 = p[5 * BLOCK + threadIdx.x];
}
// ... and five 4-byte planes behind them: pixel column, row, index in the rank's buffer, sample number, rays of the pixel so far
template <int BLOCK>
DEV void park_put_int(uint32_t off, int k, uint32_t v) { *(RT_LDS uint32_t *)(lds_raw + off + (24u + (uint32_t)k) * (uint32_t)BLOCK * 4u + threadIdx.x * 4u) = v; }
template <int BLOCK>
DEV uint32_t park_get_int(uint32_t off, int k) { return *(const RT_LDS uint32_t *)(lds_raw + off + (24u + (uint32_t)k) * (uint32_t)BLOCK * 4u + threadIdx.x * 4u); }
constexpr size_t kParkBytesPerThread = 12 * 8 + 5 * 4;  // col, throughput, accumulated: 9 doubles; RNG: 6 words; 5 counters
template <int STRICT, class T>
__global__ __launch_bounds__(T::BLOCK, T::MIN_WAVES) void render_kernel(DeviceScene sc, RenderArgs a)
{
    // What the launcher never stages for this instantiation is said here at compile time (launch_one places tables for
    // BVH worlds only, the sphere / material rows of primitive worlds only for the library-tree kernel, the big tables of
    // composite worlds only for the 768-thread workgroup): the LDS side of those row accessors folds away, and a
    // wave-uniform row of a list kernel feeds the vector instructions straight from the scalar registers it was loaded
    // into instead of being copied into vector registers to meet the other path (C4 2268 -> 2472 Msamples/s).
    if constexpr (T::WORLD != 0 || (!T::COMPOSITE && !T::FAST)) {
        sc.lds_quad_aa = sc.lds_boxes = sc.lds_objects = sc.lds_xforms = sc.lds_media = sc.lds_materials = sc.lds_perlin = kNone;
        sc.lds_spheres_tab = sc.lds_group_boxes = sc.lds_mspheres = sc.lds_msphere_aux = sc.lds_sphere_aux = kNone;
    } else if constexpr (T::FAST) {
        sc.lds_quad_aa = sc.lds_boxes = sc.lds_objects = sc.lds_xforms = sc.lds_media = sc.lds_perlin = sc.lds_group_boxes = kNone;
        if constexpr (T::BLOCK >= kBigBlock) {  // launched only with all of its rows staged (launch_one)
            __builtin_assume(sc.lds_mspheres != kNone && sc.lds_msphere_aux != kNone && sc.lds_spheres_tab != kNone);
            __builtin_assume(sc.lds_sphere_aux != kNone && sc.lds_materials != kNone);
        }
    } else {
        sc.lds_mspheres = sc.lds_msphere_aux = sc.lds_sphere_aux = kNone;
        if constexpr (T::BLOCK < kBigBlock) sc.lds_spheres_tab = kNone;
        if constexpr (!T::RICH) sc.lds_perlin = kNone;
        if constexpr (T::BATCH && T::BLOCK >= kBigBlock) {  // the deep kernel is launched only with all of these staged (launch_one)
            __builtin_assume(sc.lds_boxes != kNone && sc.lds_objects != kNone && sc.lds_xforms != kNone);
            __builtin_assume(sc.lds_media != kNone && sc.lds_materials != kNone && sc.lds_perlin != kNone);
            __builtin_assume(sc.lds_spheres_tab != kNone && sc.lds_group_boxes != kNone);
            if constexpr (T::SEG) __builtin_assume(sc.lds_fast_order != kNone && sc.lds_seg_media != kNone && sc.lds_seg_cand != kNone);
        }
    }
    // ---- chip-resident working set ----
    NodeView nv{};
    uint16_t *queue = nullptr;
    if constexpr (T::WORLD == 0) {
        // BVH nodes in LDS, one 72-byte row each (see lds_node_f64 for the layout and why 72)
        nv.global = sc.nodes;
        nv.in_lds = (T::BATCH && T::BLOCK >= kBigBlock) ? true : a.lds_nodes != 0;  // the deep kernel: always (launch_one)
        if constexpr (T::FAST) {
            {  // the library's own tree: rows copied as they are (always staged: see walk_node_fast)
                const uint32_t words = sc.n_fast_nodes * (kFastNodeBytes / 4u);
                uint32_t *dst = reinterpret_cast<uint32_t *>(lds_raw);
                const uint32_t *src = reinterpret_cast<const uint32_t *>(sc.fast_rows);
                for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) dst[k] = src[k];
                nv.n = sc.n_fast_nodes;
                auto stage = [](uint32_t off, const void *table, uint32_t bytes) {
                    if (off == kNone) return;
                    uint32_t *d2 = reinterpret_cast<uint32_t *>(lds_raw + off);
                    const uint32_t *s2 = static_cast<const uint32_t *>(table);
                    for (uint32_t w = threadIdx.x; w < bytes / 4u; w += blockDim.x) d2[w] = s2[w];
                };
                stage(sc.lds_mspheres, sc.mspheres, sc.n_mspheres * (uint32_t)sizeof(MSphereGeom));
                stage(sc.lds_msphere_aux, sc.msphere_aux, sc.n_mspheres * (uint32_t)sizeof(SphereAux));
                stage(sc.lds_spheres_tab, sc.spheres, sc.n_spheres * (uint32_t)sizeof(SphereGeom));
                stage(sc.lds_sphere_aux, sc.sphere_aux, sc.n_spheres * (uint32_t)sizeof(SphereAux));
                stage(sc.lds_materials, sc.materials, sc.n_materials * (uint32_t)sizeof(MaterialRec));
                __syncthreads();
            }
        } else if constexpr (T::SEG) {
            // segmented walk: the library's tree over the surface leaves (rows as they are), the leaf positions per node, the media
            auto copy = [](uint32_t off, const void *table, uint32_t bytes) {
                uint32_t *dst = reinterpret_cast<uint32_t *>(lds_raw + off);
                const uint32_t *src = static_cast<const uint32_t *>(table);
                for (uint32_t w = threadIdx.x; w < bytes / 4u; w += blockDim.x) dst[w] = src[w];
            };
            copy(0u, sc.fast_rows, sc.n_fast_nodes * kFastNodeBytes);
            copy(sc.lds_fast_order, sc.fast_order, sc.n_fast_nodes * (uint32_t)sizeof(FastOrder));
            copy(sc.lds_seg_media, sc.seg_media, sc.n_seg_media * (uint32_t)sizeof(SegMedium));
            copy(sc.lds_seg_cand, sc.seg_cand, sc.n_seg_cand * (uint32_t)sizeof(SegCandidate));
            nv.n = sc.n_fast_nodes;
        } else if (nv.in_lds) {
            const uint32_t n = sc.n_world_nodes;
            for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
                BvhNodeRec node = sc.nodes[k];
                double *row = reinterpret_cast<double *>(lds_raw + k * kLdsNodeBytes);
                uint32_t *words = reinterpret_cast<uint32_t *>(lds_raw + k * kLdsNodeBytes + 48u);
                row[0] = node.xlo; row[1] = node.xhi; row[2] = node.ylo; row[3] = node.yhi; row[4] = node.zlo; row[5] = node.zhi;
                words[0] = node.a; words[1] = node.b; words[2] = node.escape;
            }
            nv.n = n;
            __syncthreads();
        }
    }
    if constexpr (T::COMPOSITE) {
        // small scenes: the tables of the composite leaf test, word by word, behind the node rows (see DeviceScene)
        auto stage = [](uint32_t off, const void *table, uint32_t bytes) {
            if (off == kNone) return;
            uint32_t *dst = reinterpret_cast<uint32_t *>(lds_raw + off);
            const uint32_t *src = static_cast<const uint32_t *>(table);
            for (uint32_t w = threadIdx.x; w < bytes / 4u; w += blockDim.x) dst[w] = src[w];
        };
        stage(sc.lds_quad_aa, sc.quad_aa, sc.n_quads * (uint32_t)sizeof(AAQuad));
        stage(sc.lds_boxes, sc.boxes, sc.n_boxes * (uint32_t)sizeof(BoxRec));
        stage(sc.lds_objects, sc.objects, sc.n_objects * (uint32_t)sizeof(ObjectRec));
        stage(sc.lds_xforms, sc.xforms, sc.n_xforms * (uint32_t)sizeof(Xform));
        stage(sc.lds_media, sc.media, sc.n_media * (uint32_t)sizeof(MediumRec));
        stage(sc.lds_spheres_tab, sc.spheres, sc.n_spheres * (uint32_t)sizeof(SphereGeom));
        stage(sc.lds_group_boxes, sc.group_boxes, sc.n_group_boxes * (uint32_t)sizeof(GroupBox));
        stage(sc.lds_materials, sc.materials, sc.n_materials * (uint32_t)sizeof(MaterialRec));
        if constexpr (T::RICH) stage(sc.lds_perlin, sc.perlin, sc.n_perlin * (uint32_t)sizeof(PerlinRec));
        __syncthreads();  // uniform: every thread of the block gets here
    }
    SphereView sv{};
    if constexpr (T::WORLD == 2) {
        queue = reinterpret_cast<uint16_t *>(lds_raw) + (threadIdx.x >> 6) * (kQueueCap * 64);
        sv.global = sc.spheres;
        sv.n = sc.n_spheres;
        sv.n_padded = (sc.n_spheres + 63u) & ~63u;
        sv.in_lds = a.lds_spheres != 0;
        sv.reach = sc.scan_reach;
        sv.exact = a.exact_scan != 0;
        if (sv.in_lds) {
            sv.planes_off = ((uint32_t)T::BLOCK / 64u) * kQueueCap * 64u * (uint32_t)sizeof(uint16_t);
            double *planes = reinterpret_cast<double *>(lds_raw + sv.planes_off);
            const uint32_t np = sv.n_padded;
            for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) {
                SphereGeom g = sc.spheres[k < sv.n ? k : 0];
                planes[k] = g.cx; planes[np + k] = g.cy; planes[2 * np + k] = g.cz; planes[3 * np + k] = g.r2;
                planes[4 * np + k] = sc.sphere_scan[k < sv.n ? k : 0].k;
            }
            if (sc.lds_scan_pairs != kNone && sc.lds_scan_pairs != 0u && !a.filter_fp64 && !sv.exact) {
                sv.pairs_off = sc.lds_scan_pairs;
                sv.reach32 = sc.scan_reach32;
                v4f *rows = reinterpret_cast<v4f *>(lds_raw + sv.pairs_off);
                const uint32_t n_pairs = np / 2u, have = (uint32_t)scan32_padded_pairs(sv.n);
                for (uint32_t p = threadIdx.x; p < n_pairs; p += blockDim.x) {
                    SphereScanPair pr{{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {__builtin_inff(), __builtin_inff()}};  // never passes
                    if (p < have) {
                        pr = sc.sphere_scan32[p];
                        // a run's rows keep their varying coordinates in the cx and cz slots (scene_builder.cpp cut_scan_segments): back
                        uint32_t axis = kScanAxisNone;
                        for (uint32_t seg = 0; seg < sc.n_scan_segments; seg++) {
                            const ScanSegment sg = sc.scan_segments[seg];
                            if (p / kScanTripPairs - sg.first_trip < sg.n_trips) axis = sg.axis;
                        }
                        for (int h = 0; h < 2; h++) {
                            if (axis == 0u) { const float t = pr.cx[h]; pr.cx[h] = pr.cy[h]; pr.cy[h] = t; }
                            if (axis == 2u) { const float t = pr.cz[h]; pr.cz[h] = pr.cy[h]; pr.cy[h] = t; }
                        }
                    }
                    rows[p] = v4f{pr.cx[0], pr.cx[1], pr.cy[0], pr.cy[1]};
                    rows[n_pairs + p] = v4f{pr.cz[0], pr.cz[1], pr.k[0], pr.k[1]};
                }
            }
            // the window spans of the scan's trips (scan_filtered32), from behind the segment records
            if (sc.lds_scan_spans != kNone && sc.lds_scan_spans != 0u) {
                const ScanTripSpan *from = reinterpret_cast<const ScanTripSpan *>(sc.scan_segments + 2u * sc.n_scan_segments);
                ScanTripSpan *to = reinterpret_cast<ScanTripSpan *>(lds_raw + sc.lds_scan_spans);
                for (uint32_t t = threadIdx.x; t < sc.n_scan_window_trips; t += blockDim.x) to[t] = from[t];
            }
            __syncthreads();
        }
    }

    // ---- persistent waves: every lane pulls pixels from one atomic cursor until the frame is done ----
    // Slots are numbered tile-major (8x8 tiles, row-major inside a tile) so that lanes refilled together
    // start on neighbouring pixels; a slot outside the frame is simply skipped.
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tiles_x = ((uint32_t)a.width + 7u) >> 3;
    // the work queue: tile-major slots of this rank's rows
    const uint32_t total_slots = tiles_x * (((uint32_t)a.rows_owned + 7u) >> 3) * 64u;
    const CameraRec *__restrict__ cam = sc.camera;

    // this wave's role (wave-uniform): serve the list of heavy pixels first, a few at a time (RenderArgs::heavy_list)
    bool heavy_mode = T::ROLES && a.heavy_list != nullptr && (int)(threadIdx.x >> 6) < a.heavy_waves;
    bool heavy_dry = false;
    const uint32_t heavy_total = heavy_mode ? *(const RT_CONST uint32_t *)(uintptr_t)a.heavy_count : 0u;
    const uint32_t super_total = (heavy_mode && a.super_list) ? *(const RT_CONST uint32_t *)(uintptr_t)a.super_count : 0u;
    bool solo_phase = heavy_mode && a.super_list != nullptr;  // this wave still looks at the list of the longest chains first (RenderArgs::super_list)
    bool solo_hold = false;  // ... and holds one of them: no other pixel joins it
    // Pixels per serving wave: no more than it takes to start every listed pixel at once (a rank's stripes of a split frame list
    // few, and a chain is shortest with the wave to itself), at most what the launcher allows; the grouped scan of sphere lists
    // deals lanes in powers of two.
    int super_ppw = a.super_ppw, heavy_ppw = a.heavy_ppw;
    if (heavy_mode && a.adaptive_ppw) {
        const uint32_t serving = gridDim.x * (uint32_t)a.heavy_waves;
        auto fit = [&](uint32_t total, int cap) {
            int p = (int)((total + serving - 1u) / serving);
            p = p < 1 ? 1 : p;
            if (T::WORLD == 2) {
                int q = 1;
                while (q < p) q *= 2;
                p = q;
            }
            return p > cap ? cap : p;
        };
        // (both tiers by the two lists' sum: with the first tier alone in view a full C2 frame would serve it two to a wave and
        // start the second tier later -- 193 -> 197 ms)
        super_ppw = fit(super_total + heavy_total, a.super_ppw);
        heavy_ppw = fit(super_total + heavy_total, a.heavy_ppw);
    }
    if (heavy_mode) {
        if (a.heavy_priority == 1) __builtin_amdgcn_s_setprio(1);
        else if (a.heavy_priority == 2) __builtin_amdgcn_s_setprio(2);
        else if (a.heavy_priority == 3) __builtin_amdgcn_s_setprio(3);
    }
    bool active = false, exhausted = false;
    int i = 0, j = 0;
    size_t local = 0;
    Xorwow rng{0, 0, 0, 0, 0, 0};
    Vec col = mk(0.0, 0.0, 0.0);
    Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
    Ray ray{};
    int sample = 0, depth = 0;
    uint32_t wave_rays = 0;  // rays of the whole wave (uniform)
    // adaptive sampling: samples the pixel had before this launch, its sum of y^2, and the samples this wave has taken (uniform)
    [[maybe_unused]] uint32_t ad_before = 0;
    [[maybe_unused]] double ad_q = 0.0;
    [[maybe_unused]] unsigned long long wave_samples = 0;

    uint32_t pix_rays = 0;  // rays this lane's current pixel has traced so far
    // 8x8 tile of the current pixel, in the numbering of tile_cost and of primary_lists: the rehearsal books costs under it and a
    // primary round reads the tile's list by it, so every path of the refill that hands a lane a pixel sets it -- the tile
    // queue, the heavy list and the super list (the listed pixels' from their row and column)
    uint32_t my_tile = 0;
    int boost_left = 0;     // extra overdue-only passes still allowed before the next pixel-parallel pass
    [[maybe_unused]] bool primary_since_scan = false;  // ... and one has run since the wave's last pixel-parallel pass
    // fewest fresh lanes for which a round pays beside a pass over this list (kPrimaryRoundCost): 16 for C2's 485 spheres
    [[maybe_unused]] const int primary_break_even = (int)((64u * kPrimaryRoundCost) / (kPrimaryPassFixed + (sc.n_spheres * kPrimaryPassPerSphere100) / 100u));
    [[maybe_unused]] bool primary_last = false;  // the last trip of the main loop was a primary round (wave-uniform): the boost count stands
    // BVH worlds: per-lane resumable traversal (see Walk) and the hit it has found so far
    Walk walk{};
    walk.state = kNone;  // no walk in progress
    HitInfo walk_best;
    walk_best.t = 0.0;
    walk_best.ref = kNone;
    walk_best.obj = kNone;
    [[maybe_unused]] SegState seg{0u, kSegEnd, 0u};  // segmented walk: hi == kSegEnd also means "nothing more to walk" for an idle lane

    // the rehearsal (RenderArgs::probe): a pixel's rays are booked where it ends, or where it reaches the ray cap
    const uint32_t probe_cap = (!T::ADAPTIVE && a.probe && a.probe_ray_cap > 0) ? (uint32_t)a.probe_ray_cap : 0xFFFFFFFFu;  // (rehearsals run the plain kernels)
    auto book_cost = [&](uint32_t rays) {
        if constexpr (T::PARK) {  // the pixel's index and its tile come back from LDS
            local = (size_t)park_get_int<T::BLOCK>(sc.lds_park, 2);
            const uint32_t row = (uint32_t)local / (uint32_t)a.width, column = (uint32_t)local % (uint32_t)a.width;
            my_tile = (row >> 3) * tiles_x + (column >> 3);
        }
        if (a.tile_cost) atomicAdd(a.tile_cost + my_tile, rays);
        if (a.pix_cost) a.pix_cost[local] = rays;
    };

#if RT_PHASES
    PhaseSums ph{};
    const unsigned long long ph_start = __builtin_readcyclecounter();
    bool ph_serving = heavy_mode;  // RT_PHASES == 2: only the waves serving heavy pixels report, and only that part of their life
#endif
    for (;;) {
        // A pixel that has used up its ray budget is "overdue": its samples cannot be spread over lanes (one
        // sequential RNG stream per pixel), and at one ray per pixel-parallel pass it would finish long after the
        // rest of the frame.  So after every pixel-parallel pass the wave inserts up to `boost_rounds` extra passes
        // in which only the overdue lanes advance, each of their rays scanned cooperatively by all 64 lanes.
        unsigned long long overdue = 0;
        bool boost = false;
        if constexpr (T::WORLD == 2) {
            overdue = __ballot(active && pix_rays >= a.ray_budget);
            if (a.overdue_priority) {  // diagnostic alternative: keep the pixel-parallel scan but raise this wave's issue priority
                if (overdue) __builtin_amdgcn_s_setprio(3);
                else __builtin_amdgcn_s_setprio(0);
                overdue = 0;
            }
            if (primary_last) {  // a primary round is no pixel-parallel pass: the overdue lanes' extra passes follow the scan, as ever
                overdue = 0;
            } else {
                boost = overdue != 0 && boost_left > 0;
                if (boost) boost_left--;
                else boost_left = a.boost_rounds;
            }
            primary_last = false;
        }

        const bool from_list = heavy_mode && !heavy_dry;  // this refill takes heavy pixels off the list
        if (solo_hold && !__any(active)) solo_hold = false;
        if (!exhausted && !boost && (!heavy_mode || from_list) && !solo_hold) {
            unsigned long long need = __ballot(!active);
            // pixels_per_wave < 64: only the first lanes take pixels.  Sphere-list kernel: the others lend themselves to the
            // grouped scan; BVH kernels: the few rays have the wave's phases to themselves (shorter chain per pixel).
            const bool from_super = from_list && solo_phase;  // one of the longest chains, alone in this wave until it is done
            const int ppw = from_super ? super_ppw : (from_list ? heavy_ppw : a.pixels_per_wave);
            if (ppw < 64) need &= (1ull << ppw) - 1ull;
            if (need) {
                PH_BEGIN();
                [[maybe_unused]] const bool ph_was_idle = !active;
                const uint32_t cnt = (uint32_t)__popcll(need);
                const uint32_t queue_len = from_super ? super_total : (from_list ? heavy_total : total_slots);
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(from_super ? a.super_cursor : (from_list ? a.heavy_cursor : a.cursor), cnt);
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                if (base + cnt >= queue_len) {
                    if (from_super) solo_phase = false;
                    else if (from_list) heavy_dry = true;
                    else exhausted = true;
                }
                const uint32_t slot = base + (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
                if (((need >> lane) & 1ull) && slot < queue_len) {
                    // heaviest tiles first when the launcher has ranked them (see rt_render_launch); else row-major
                    const uint32_t w = slot & 63u;
                    uint32_t tile = (a.tile_order && !from_list) ? a.tile_order[slot >> 6] : slot >> 6;
                    int pi = (int)((tile % tiles_x) * 8u + (w & 7u));
                    int lr = (int)((tile / tiles_x) * 8u + (w >> 3));
                    bool take = pi < a.width && lr < a.rows_owned;
                    if (from_list) {  // listed pixels: compact index -> row, column
                        const uint32_t loc = from_super ? a.super_list[slot] : a.heavy_list[slot];
                        lr = (int)(loc / (uint32_t)a.width);
                        pi = (int)(loc % (uint32_t)a.width);
                        tile = ((uint32_t)lr >> 3) * tiles_x + ((uint32_t)pi >> 3);
                        take = true;
                    } else if (a.pix_class && take) {
                        take = a.pix_class[(size_t)lr * (size_t)a.width + (size_t)pi] == 0;  // a listed pixel: the serving waves take it
                    }
                    if constexpr (T::ADAPTIVE) {  // stopped by the rule in an earlier launch of this frame: it stays as it is
                        if (take && a.ad_mark[(size_t)lr * (size_t)a.width + (size_t)pi] != 0) take = false;
                    }
                    if (take) {
                        i = pi;
                        j = owned_row(lr, a.stripe_rows, a.rank, a.world_size);
                        local = (size_t)lr * (size_t)a.width + (size_t)pi;
                        if constexpr (T::ADAPTIVE) {
                            ad_before = a.ad_n[local];
                            ad_q = a.ad_q[local];
                        }
                        rng.d = a.state[0 * (size_t)a.n_pixels + local];
                        rng.v0 = a.state[1 * (size_t)a.n_pixels + local];
                        rng.v1 = a.state[2 * (size_t)a.n_pixels + local];
                        rng.v2 = a.state[3 * (size_t)a.n_pixels + local];
                        rng.v3 = a.state[4 * (size_t)a.n_pixels + local];
                        rng.v4 = a.state[5 * (size_t)a.n_pixels + local];
                        col = mk(0.0, 0.0, 0.0);
                        sample = 0;
                        int sum_spp = a.spp_before;  // samples in the pixel's running sum
                        // behind a rehearsal that kept its samples: a pixel it stopped at the ray cap saved nothing, it starts from
                        // its first sample (RenderArgs::resumed_spp)
                        if constexpr (!T::ADAPTIVE) {  // (adaptive frames resume from nothing: launch_one)
                            if (a.resumed_spp > 0 && a.probe_ray_cap > 0 && a.pix_cost[local] >= (uint32_t)a.probe_ray_cap) {
                                sample = -a.resumed_spp;
                                sum_spp -= a.resumed_spp;
                            }
                        }
                        if (a.accum && sum_spp > 0)  // progressive: continue the running sum in the same order
                            col = mk(a.accum[local * 3 + 0], a.accum[local * 3 + 1], a.accum[local * 3 + 2]);
                        throughput = mk(1.0, 1.0, 1.0);
                        accumulated = mk(0.0, 0.0, 0.0);
                        depth = 0;
                        pix_rays = 0;
                        my_tile = tile;
                        ray = camera_ray(cam, i, j, a.width, a.height, rng);
                        active = true;
                        if constexpr (T::PARK) {
                            park_put_int<T::BLOCK>(sc.lds_park, 0, (uint32_t)i);
                            park_put_int<T::BLOCK>(sc.lds_park, 1, (uint32_t)j);
                            park_put_int<T::BLOCK>(sc.lds_park, 2, (uint32_t)local);
                            park_put_int<T::BLOCK>(sc.lds_park, 3, (uint32_t)sample);
                            park_put_int<T::BLOCK>(sc.lds_park, 4, 0u);
                            park_put_vec<T::BLOCK>(sc.lds_park, 0, col);
                            park_put_vec<T::BLOCK>(sc.lds_park, 3, throughput);
                            park_put_vec<T::BLOCK>(sc.lds_park, 6, accumulated);
                            (park_put_rng<T::BLOCK>)(sc.lds_park, rng);  // (in parentheses: no argument-dependent lookup, which would find the first pass's from the second)
                        }
                        if constexpr (T::WORLD == 0) {
                            walk_begin<T::FAST || T::SEG>(walk, ray, DBL_MAX);
                            if constexpr (T::SEG) {  // "between walks", before the first one: seg_advance at the head of the next round
                                seg = SegState{0u, 0u, 0u};
                                walk.state = kNone;
                            }
                        }
                    }
                }
                if (from_super && __any(active)) solo_hold = true;
                PH_END(3, ph_was_idle && active);
            }
        }
        const unsigned long long live = __ballot(active);
        if (!live) {
            if (heavy_mode && heavy_dry) {  // the list is done and so are this wave's heavy pixels: join the tile queue
                heavy_mode = false;
                __builtin_amdgcn_s_setprio(0);
#if RT_PHASES == 2
                ph_flush(a, ph, ph_start, lane);
                ph_serving = false;
#endif
                continue;
            }
            if (exhausted) break;
            continue;
        }

        // ---- one ray segment for every lane in `todo` ----
        unsigned long long todo = live;
        HitInfo h;
        h.t = 0.0;
        h.ref = kNone;
        h.obj = kNone;
        bool hit = false;
        if constexpr (T::WORLD == 2) {
            if (boost) todo = overdue;
            // ---- primary round (r18): camera rays against their tile's candidate list instead of the whole list ----
            // Where the wave would run the pixel-parallel scan, the lanes whose ray is a camera ray (depth == 0) and whose tile has a
            // list (primary_cull_rule.h: every sphere the reference could accept for ANY camera ray of the tile) run the reference's
            // test on the listed spheres alone, in list order, and go on to the shading below; the other lanes wait.  Rounds repeat
            // -- a lane whose path ended holds a new camera ray -- while nobody needs the scan; otherwise one round per pass, if it pays.
            const bool scan_wave = !boost && a.pixels_per_wave >= 64 && __popcll(live) >= a.coop_threshold;
            if (scan_wave && a.primary_lists != nullptr && a.max_depth > 0) {
                const bool camera = active && depth == 0;
                const unsigned long long cameras = __ballot(camera);
                // A round that leaves lanes waiting must pay (primary_break_even), is the only one since the last scan pass (sky lanes
                // are fresh again after every round: without this a mixed wave holds its secondary rays back round after round),
                // and delays no pixel whose chain of rays is long enough to decide when the frame ends (kPrimaryLongChain).
                const bool may_round = !primary_since_scan && __popcll(cameras) >= primary_break_even &&
                                       !__any(active && pix_rays > kPrimaryLongChain * (uint32_t)(sample + 16));
                if (cameras == live || may_round) {
                    PH_BEGIN();
                    // the list's first half; the second is fetched where a lane gets that far (eight registers of list words at once
                    // cost the adaptive instantiation two spills)
                    uint4 wa = uint4{kPrimaryNoList, 0u, 0u, 0u};
                    const uint4 *row = reinterpret_cast<const uint4 *>(a.primary_lists + (size_t)my_tile * kPrimaryListWords);
                    if (camera) wa = row[0];
                    uint32_t n_listed = wa.x & 0xFFFFu;
                    const bool fresh = camera && n_listed != kPrimaryNoList;
                    const unsigned long long freshes = __ballot(fresh);
                    primary_last = freshes != 0 && (freshes == live || (may_round && __popcll(freshes) >= primary_break_even));
                    if (primary_last) primary_since_scan = true;
                    if (primary_last) {
                        todo = freshes;
                        if (!fresh) n_listed = 0u;
                        n_listed = n_listed < kPrimaryListMax ? n_listed : kPrimaryListMax;
                        const double ra = dot(ray.d, ray.d);
                        double closest = DBL_MAX;
                        uint32_t best_k = kNone;
#if RT_PHASES
                        ph.n[23] += 1ull;
                        ph.l[23] += (unsigned long long)__popcll(freshes);
                        for (uint32_t e = n_listed, off = 32; off > 0; off >>= 1) {
                            e += (uint32_t)__shfl_xor((int)e, (int)off, 64);
                            if (off == 1) ph.t[15] += e;
                        }
#endif
                        for (uint32_t s = 0; __any(s < n_listed); s++) {
                            // the next entry: the half list moves down by one uint16; entry 7 is the first of the second half
                            if (s == 7u) {
                                if (s < n_listed) wa = row[1];
                            } else {
                                wa.x = __builtin_amdgcn_alignbit(wa.y, wa.x, 16); wa.y = __builtin_amdgcn_alignbit(wa.z, wa.y, 16);
                                wa.z = __builtin_amdgcn_alignbit(wa.w, wa.z, 16); wa.w >>= 16;
                            }
                            if (s < n_listed) {
                                const uint32_t k = wa.x & 0xFFFFu;
                                SphereGeom g;
                                if (sv.in_lds) {
                                    const RT_LDS double *pl = (const RT_LDS double *)(lds_raw + sv.planes_off);
                                    g = SphereGeom{pl[k], pl[sv.n_padded + k], pl[2u * sv.n_padded + k], pl[3u * sv.n_padded + k]};
                                } else {
                                    g = sc.spheres[k];
                                }
                                double t;
                                if (sphere_test(ray.o - mk(g.cx, g.cy, g.cz), ray.d, ra, g.r2, 0.001, closest, t)) {
                                    closest = t;
                                    best_k = k;
                                }
                            }
                        }
                        hit = best_k != kNone;
                        if (hit) {
                            h.t = closest;
                            h.ref = make_ref(REF_SPHERE, best_k);
                            h.obj = kNone;
                        }
                    }
#if RT_PHASES
                    if (primary_last) {
                        asm volatile("" ::"v"(h.t), "v"(h.ref));
                        ph.t[23] += __builtin_readcyclecounter() - ph_t0;
                    }
#endif
                }
            }
            if (primary_last) {
                // (nothing more to search: `todo`, `hit` and `h` are set)
            } else if (scan_wave) {
                primary_since_scan = false;
                PH_BEGIN();
#if RT_PHASES
                ScanSums ss{};
#endif
                if (a.exact_scan || a.filter_fp64) {
                    if (active) hit = a.exact_scan ? scan_uniform(sc, queue, lane, ray, 0.001, DBL_MAX, h)
                                      : sv.in_lds  ? scan_filtered<true>(sc, sv.planes_off, sv.n_padded, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS)
                                                   : scan_filtered<false>(sc, 0u, 0u, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS);
                } else if (a.scan_windows) {  // some run has a window table: the windows are the wave's, formed by all 64 lanes (scan_filtered32)
                    hit = sv.in_lds ? scan_filtered32<true, true>(sc, active, sv.planes_off, sv.n_padded, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS)
                                    : scan_filtered32<false, true>(sc, active, 0u, 0u, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS);
                } else {
                    if (active) hit = sv.in_lds ? scan_filtered32<true, false>(sc, true, sv.planes_off, sv.n_padded, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS)
                                                : scan_filtered32<false, false>(sc, true, 0u, 0u, queue, lane, ray, 0.001, DBL_MAX, h SS_PASS);
                }
                PH_END(0, active);
#if RT_PHASES
                ph.n[19] += 1ull;  // slot 19 (no primitive pass in this kernel): live lanes of the pass, and those with a camera ray
                ph.l[19] += (unsigned long long)__popcll(live);
                ph.t[19] += (unsigned long long)__popcll(__ballot(active && depth == 0));
                {  // the sums are wave-uniform (the packed scan runs in all lanes, the others in the active ones): take them from the first active lane
                    const int src = __ffsll((long long)__ballot(active)) - 1;
                    if (src >= 0) {
                    const auto rl = [src](uint32_t v) { return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)v, src); };
                    ph.n[12] += rl(ss.groups);  ph.l[12] += rl(ss.taken);        ph.t[12] += rl(ss.spheres);
                    ph.n[13] += rl(ss.appends); ph.l[13] += rl(ss.behind);       ph.t[13] += rl(ss.drain_cycles);
                    ph.n[15] += rl(ss.drains);  ph.l[15] += rl(ss.drain_iters);
                    ph.n[14] += rl(ss.win_runs); ph.l[14] += rl(ss.win_trips);   ph.t[14] += rl(ss.win_cycles);
                    ph.n[7] += rl(ss.win_runs) ? 1ull : 0ull; ph.l[7] += rl(ss.win_ranges); ph.t[7] += rl(ss.win_lane_trips);
                    }
                }
#endif
            } else {
                PH_BEGIN();
#if RT_PHASES
                GroupedSums gs{};
#endif
                if (sv.in_lds && !a.coop_single) scan_grouped(sv, queue, lane, todo, ray, 0.001, DBL_MAX, h, hit GS_PASS);
                else scan_cooperative(sv, lane, todo, ray, 0.001, DBL_MAX, h, hit);
                PH_END(1, (todo >> lane) & 1ull);
#if RT_PHASES
                if (gs.rays) {  // a grouped pass through the filter: every lane ran it and holds the same sums
                    ph.n[16] += 1ull;       ph.l[16] += gs.rays;     ph.t[16] += gs.tests;
                    ph.n[17] += gs.drains;  ph.l[17] += gs.lane_max; ph.t[17] += gs.survivors;
                    ph.l[18] += gs.filter_cycles; ph.t[18] += gs.test_cycles;
                }
#endif
            }
        }
        bool thin = false;
        if constexpr (T::WORLD == 0 && !T::COMPOSITE) {
            // Frame tail of a sphere world: the queue is dry and few lanes are left -- scan instead of walking (scan_grouped_ms).
            // The same closest hit as the walk: no leaf draws random numbers, and the launcher sets coop_threshold = 0 where a
            // hit could lie outside its leaf's box (a moving sphere at a ray time outside its interval: hits_stay_in_boxes).
            thin = sc.ms_planes != nullptr && exhausted && __popcll(live) < a.coop_threshold;
            if (thin) {
                PH_BEGIN();
                scan_grouped_ms(sc, lane, live, ray, 0.001, DBL_MAX, h, hit);
                walk.state = kNone;  // a walk in progress is dropped: the scan has covered every leaf
                PH_END(1, active);
            }
        }
        if constexpr (T::WORLD == 0) if (!thin) {
            // Traversal burst: every walking lane advances up to kBurst nodes.  Lanes whose walk is complete
            // wait for shading; they are shaded once enough of them have gathered (or nobody is walking any
            // more), then start their next ray and rejoin the walkers.
            // Inner nodes and leaves run in separate phases so that the (long, branchy) leaf tests execute with
            // many lanes at once instead of trailing every node visit with a few.
            // node/leaf phase pairs per look at the shading queue: measured optimum 6 for primitive worlds (C3: 8 -> 6 is
            // +7 %, 4 is -1 %), 4 for composite ones (C5: +6 %; C4 indifferent)
            const int n_rounds = T::BATCH ? a.rounds : (T::COMPOSITE ? kRoundsComposite : (T::FAST ? kRoundsFast : kRounds));
            for (int round = 0; round < n_rounds; round++) {
                if constexpr (T::SEG) {
                    // between two walks (a new ray, or a walk that was not the ray's last has ended): the media that are due, then
                    // the next walk (seg_advance) -- the one place where media are tested and draw
                    const bool between = active && walk.state == kNone && seg.hi != kSegEnd;
                    if (__any(between)) {
                        PH_BEGIN();
#if RT_PHASES
                        const bool ph_again = between && seg.hi != 0u;  // not the ray's first time here: a limited walk has ended
#endif
                        if (between) seg_advance<T>(sc, ray, walk, walk_best, rng, seg PH_PASS);
                        PH_END(17, between);
#if RT_PHASES
                        if (__any(ph_again)) PH_END(12, ph_again);
#endif
                    }
                }
                for (int step = 0; step < (T::COMPOSITE ? a.node_burst : kBurst); step++) {
                    const bool mover = walk_moving(walk.state);
                    [[maybe_unused]] bool limited_walks = false;
                    if constexpr (T::SEG) limited_walks = __any(mover && seg.hi != kSegEnd);
                    const int movers = __popcll(__ballot(mover));
                    const int parked = __popcll(__ballot(walk_parked(walk.state)));
                    // most walkers are waiting at leaves: go test them.  A composite leaf (box, instance, medium) costs
                    // tens of node steps, so there the leaf phase waits for a larger share of the walkers.
                    if (movers == 0 || movers * (T::COMPOSITE ? a.park_ratio : 1) < parked) break;
                    {
                        PH_BEGIN();
#if RT_PHASES
                        if (limited_walks) PH_END(13, mover && seg.hi != kSegEnd);
#endif
                        if (mover) {
                            if constexpr (T::FAST) {
                                walk_node_fast(ray, 0.001, walk);
                                PH_COUNT(14);
                                if (walk_moving(walk.state)) {
                                    walk_node_fast(ray, 0.001, walk);
                                    PH_COUNT(14);
                                }
                            } else if constexpr (T::SEG) {
                                if (limited_walks) {  // some lane of the wave is on its way to a medium (wave-uniform, rare)
                                    walk_node_seg(sc, ray, 0.001, walk, seg.hi);
                                    PH_COUNT(14);
                                    if (walk_moving(walk.state)) {
                                        walk_node_seg(sc, ray, 0.001, walk, seg.hi);
                                        PH_COUNT(14);
                                    }
                                } else {
                                    walk_node_open(ray, 0.001, walk);
                                    PH_COUNT(14);
                                    if (walk_moving(walk.state)) {
                                        walk_node_open(ray, 0.001, walk);
                                        PH_COUNT(14);
                                    }
                                }
                            } else
                            {
                                walk_node<T::BATCH>(nv, ray, 0.001, walk);
                                PH_COUNT(14);
                            }
                            // Primitive worlds (deep BVH, cheap leaves): a second visit before the next look at the
                            // wave's state -- the ballots and counts that steer the phases cost a fifth of a node visit.
                            // Not for composite worlds: the Cornell box's tree is three levels deep (measured -17 %).
                            // Kind-batched kernels run on deep trees too: the same second visit (C5 +x %).
                            if constexpr ((!T::COMPOSITE || T::BATCH) && !T::FAST && !T::SEG) {
                                if (walk_moving(walk.state)) {
                                    walk_node<T::BATCH>(nv, ray, 0.001, walk);
                                    PH_COUNT(14);
                                }
                            }
                        }
                        PH_END(0, mover);
                    }
                }
                if constexpr (T::BATCH) {
                    const bool at_leaf = walk_parked(walk.state);
                    if (__any(at_leaf)) {
                        const uint32_t kind = (walk.state >> kWalkKindShift) & 3u;  // of the pending leaf (walk_node, walk_leaf_pass)
                        // everything is served in the last round before shading is looked at again, and when nobody walks
                        const bool serve_all = round + 1 == n_rounds || !__any(walk_moving(walk.state));
#define RT_LEAF_PASS(K, SLOT)                                                                                          \
                        {                                                                                              \
                            const bool mine = at_leaf && kind == (K);                                                  \
                            const int waiting = __popcll(__ballot(mine));                                              \
                            if (waiting > 0 && (serve_all || waiting >= a.leaf_batch)) {                               \
                                PH_BEGIN();                                                                            \
                                if (mine) walk_leaf_pass<T, (K)>(sc, nv, ray, 0.001, walk, walk_best, rng,             \
                                                                 T::SEG ? seg_pending_leaf(walk.state) : walk_pending_leaf(nv, walk.state) PH_PASS, \
                                                                 false, false, 0.0, kNone, seg.lo, seg.hi);            \
                                PH_END(SLOT, mine);                                                                    \
                            }                                                                                          \
                        }
                        RT_LEAF_PASS(LK_BOX, 16)
                        if constexpr (T::MEDIA && !T::SEG) RT_LEAF_PASS(LK_MEDIUM, 17)  // segmented walk: no medium is a leaf of the tree
                        {  // instances and groups: the whole wave takes part (walk_object_pass)
                            const bool mine = at_leaf && kind == LK_OBJECT;
                            const int waiting = __popcll(__ballot(mine));
                            if (waiting > 0 && (serve_all || waiting >= a.object_batch)) {
                                PH_BEGIN();
                                walk_object_pass<T>(sc, nv, ray, 0.001, walk, walk_best, rng,
                                                    mine ? (T::SEG ? seg_pending_leaf(walk.state) : walk_pending_leaf(nv, walk.state)) : kNone, mine,
                                                    lane PH_PASS, seg.lo, seg.hi);
                                PH_END(18, mine);
                            }
                        }
                        RT_LEAF_PASS(LK_PRIM, 19)
#undef RT_LEAF_PASS
                    }
                } else {
                    const bool at_leaf = walk_parked(walk.state);
                    PH_BEGIN();
                    if (at_leaf) {
                        if constexpr (T::FAST) walk_leaves_fast(sc, ray, 0.001, walk, walk_best);
                        else walk_leaves<T>(sc, nv, ray, 0.001, walk, walk_best, rng PH_PASS);
                    }
                    if (__any(at_leaf)) PH_END(1, at_leaf);
                }
                if constexpr (T::SEG) {
                    if (!__any(walk.state != kNone || (active && seg.hi != kSegEnd))) break;
                } else
                if (!__any(walk.state != kNone)) break;
            }
            // segmented walk: a lane between two walks is still on its way, not waiting to be shaded
            const unsigned long long walkers = T::SEG ? __ballot(walk.state != kNone || (active && seg.hi != kSegEnd)) : __ballot(walk.state != kNone);
            const unsigned long long waiting = live & ~walkers;
            const int n_wait = __popcll(waiting), n_walk = __popcll(walkers);
            todo = (n_wait >= a.shade_batch || n_wait >= n_walk) ? waiting : 0ull;
            hit = walk.any;
            h = walk_best;
        }
#if RT_PHASES
        const unsigned long long ph_ts = __builtin_readcyclecounter();
#endif
        if constexpr (T::GROUPED) {  // every ray's leaves are dealt to 64 / pixels_per_wave lanes (the launcher keeps pixels_per_wave a power of two below 64)
            PH_BEGIN();
            scan_leaves_grouped<T>(sc, lane, 6 - (__ffs(a.pixels_per_wave) - 1), todo, ray, 0.001, DBL_MAX, h, hit, rng PH_PASS);
            PH_END(1, (todo >> lane) & 1ull);
        }
        if (a.max_depth > 0) wave_rays += (uint32_t)__popcll(todo);
        [[maybe_unused]] bool sample_ends = false;
        bool mine = (todo >> lane) & 1ull;
        if (probe_cap != 0xFFFFFFFFu && a.max_depth > 0) {
            // The rehearsal stops at the decision: with this ray the pixel's count reaches the cap (RenderArgs::probe_ray_cap) -- it is
            // listed among the longest chains whatever it traces from here on, and those are what the launch would end on.  The lane
            // books the count and goes idle in mid-sample; nothing of the pixel is saved, and the rays it has counted leave the
            // wave's sum again (the frame launch traces them once more).
            uint32_t rays = pix_rays + 1u;
            if constexpr (T::PARK) rays = park_get_int<T::BLOCK>(sc.lds_park, 4) + 1u;
            const bool capped = mine && rays >= probe_cap;
            if (capped) {
                book_cost(rays);
                active = false;
                mine = false;
                if constexpr (T::SEG) seg.hi = kSegEnd;  // no pixel: nothing between walks either
            }
            wave_rays -= probe_cap * (uint32_t)__popcll(__ballot(capped));
        }
        if (mine) {
            const bool no_bounces = a.max_depth <= 0;  // R/kernel.cu:71: the bounce loop never runs, RayColor returns black
            if (!no_bounces) {
                if constexpr (T::PARK) {
                    if (a.probe) park_put_int<T::BLOCK>(sc.lds_park, 4, park_get_int<T::BLOCK>(sc.lds_park, 4) + 1u);  // only the rehearsal asks
                } else {
                    pix_rays++;
                }
            }
            if constexpr (T::WORLD == 1 && !T::GROUPED) hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng PH_PASS);
            if constexpr (T::PARK) {  // back from LDS: what the shading works on (no leaf of these worlds draws random numbers)
                throughput = park_get_vec<T::BLOCK>(sc.lds_park, 3);
                accumulated = park_get_vec<T::BLOCK>(sc.lds_park, 6);
                (park_get_rng<T::BLOCK>)(sc.lds_park, rng);
            }
            bool path_ends;
            if (no_bounces) {
                path_ends = true;
            } else if (!hit) {  // R/kernel.cu:74-79
                accumulated = accumulated + throughput * miss_value<T>(sc, cam, ray.d);
                path_ends = true;
            } else {
#if RT_PHASES
                const unsigned long long ph_a = __builtin_readcyclecounter();
#endif
                Surface s = make_surface<T>(sc, ray, h);
#if RT_PHASES
                asm volatile("" ::"v"(s.p.x), "v"(s.n.z), "v"(s.mat));
                const unsigned long long ph_b = __builtin_readcyclecounter();
                ph.t[20] += ph_b - ph_a;
                ph.l[20] += (unsigned long long)__popcll(__ballot(true));
                ph.n[20] += 1ull;
#endif
                path_ends = !shade<T>(sc, s, ray, throughput, accumulated, rng);
#if RT_PHASES
                asm volatile("" ::"v"(ray.d.x), "v"(throughput.x));
                ph.t[21] += __builtin_readcyclecounter() - ph_b;
                ph.l[21] += (unsigned long long)__popcll(__ballot(true));
                ph.n[21] += 1ull;
#endif
                if (!path_ends && ++depth >= a.max_depth) path_ends = true;  // R/kernel.cu:71,97
            }
#if RT_PHASES
            const unsigned long long ph_c = __builtin_readcyclecounter();
            if (path_ends && sample + 1 < a.spp) {
                ph.l[22] += (unsigned long long)__popcll(__ballot(true));
                ph.n[22] += 1ull;
            }
#endif
            if (path_ends) {  // R/kernel.cu:143: col += RayColor(...)
                if constexpr (T::PARK) {
                    col = park_get_vec<T::BLOCK>(sc.lds_park, 0);
                    sample = (int)park_get_int<T::BLOCK>(sc.lds_park, 3);
                }
                col = col + accumulated;
                bool more = ++sample < a.spp;
                [[maybe_unused]] bool converged = false;
                if constexpr (T::ADAPTIVE) {
                    sample_ends = true;
                    ad_q = adaptive_add_sample(ad_q, accumulated.x, accumulated.y, accumulated.z);
                    // (also at the launch's cap: the mark must be right for a later launch of the frame)
                    converged = adaptive_converged(a.rule, ad_before + (uint32_t)sample, col.x, col.y, col.z, ad_q);
                    if (converged) more = false;
                }
                if (more) {
                    if constexpr (T::PARK) {
                        park_put_vec<T::BLOCK>(sc.lds_park, 0, col);
                        park_put_int<T::BLOCK>(sc.lds_park, 3, (uint32_t)sample);
                        i = (int)park_get_int<T::BLOCK>(sc.lds_park, 0);
                        j = (int)park_get_int<T::BLOCK>(sc.lds_park, 1);
                    }
                    ray = camera_ray(cam, i, j, a.width, a.height, rng);
                    throughput = mk(1.0, 1.0, 1.0);
                    accumulated = mk(0.0, 0.0, 0.0);
                    depth = 0;
                } else if (a.probe) {
                    // the rehearsal: book the rays; where the frame launch resumes from it (RenderArgs::probe == 2), the pixel's stream
                    // and its sum so far are saved as a frame saves them, and no pixel is written
                    if constexpr (T::PARK) pix_rays = park_get_int<T::BLOCK>(sc.lds_park, 4);
                    book_cost(pix_rays);
                    if (a.probe == 2) {
                        a.state[0 * (size_t)a.n_pixels + local] = rng.d;
                        a.state[1 * (size_t)a.n_pixels + local] = rng.v0;
                        a.state[2 * (size_t)a.n_pixels + local] = rng.v1;
                        a.state[3 * (size_t)a.n_pixels + local] = rng.v2;
                        a.state[4 * (size_t)a.n_pixels + local] = rng.v3;
                        a.state[5 * (size_t)a.n_pixels + local] = rng.v4;
                        a.accum[local * 3 + 0] = col.x;
                        a.accum[local * 3 + 1] = col.y;
                        a.accum[local * 3 + 2] = col.z;
                    }
                    active = false;
                } else {
                    // R/kernel.cu:146-153: save the RNG state, average, gamma 2
                    if constexpr (T::PARK) local = (size_t)park_get_int<T::BLOCK>(sc.lds_park, 2);
                    a.state[0 * (size_t)a.n_pixels + local] = rng.d;
                    a.state[1 * (size_t)a.n_pixels + local] = rng.v0;
                    a.state[2 * (size_t)a.n_pixels + local] = rng.v1;
                    a.state[3 * (size_t)a.n_pixels + local] = rng.v2;
                    a.state[4 * (size_t)a.n_pixels + local] = rng.v3;
                    a.state[5 * (size_t)a.n_pixels + local] = rng.v4;
                    if (a.accum) {
                        a.accum[local * 3 + 0] = col.x;
                        a.accum[local * 3 + 1] = col.y;
                        a.accum[local * 3 + 2] = col.z;
                    }
                    if constexpr (T::ADAPTIVE) {  // the pixel's own n
                        const uint32_t n = ad_before + (uint32_t)sample;
                        a.ad_n[local] = n;
                        a.ad_q[local] = ad_q;
                        a.ad_mark[local] = converged ? 1 : 0;
                        col = over(col, (double)n);
                    } else {
                        col = over(col, (double)(a.spp_before + a.spp));
                    }
                    a.pixels[local * 3 + 0] = sqrt(col.x);
                    a.pixels[local * 3 + 1] = sqrt(col.y);
                    a.pixels[local * 3 + 2] = sqrt(col.z);
                    active = false;
                }
            }
#if RT_PHASES
            asm volatile("" ::"v"(ray.d.x), "v"(col.x));
            ph.t[22] += __builtin_readcyclecounter() - ph_c;  // next camera ray or pixel done (booked together)
#endif
            if constexpr (T::PARK) {
                if (active) {
                    park_put_vec<T::BLOCK>(sc.lds_park, 3, throughput);
                    park_put_vec<T::BLOCK>(sc.lds_park, 6, accumulated);
                    (park_put_rng<T::BLOCK>)(sc.lds_park, rng);  // (in parentheses: no argument-dependent lookup, which would find the first pass's from the second)
                }
            }
            if constexpr (T::WORLD == 0) {
                if (active) {
                    walk_begin<T::FAST || T::SEG>(walk, ray, DBL_MAX);
                    if constexpr (T::SEG) {
                        seg = SegState{0u, 0u, 0u};
                        walk.state = kNone;
                    }
                } else if constexpr (T::SEG) {
                    seg.hi = kSegEnd;  // no pixel: nothing between walks either
                }
            }
        }
        if constexpr (T::ADAPTIVE) wave_samples += (unsigned long long)__popcll(__ballot(sample_ends));
#if RT_PHASES
        if (todo) {
            ph.t[2] += __builtin_readcyclecounter() - ph_ts;
            ph.l[2] += (unsigned long long)__popcll(todo);
            ph.n[2] += 1ull;
        }
#endif
    }
#if RT_PHASES
    if (RT_PHASES == 1 || ph_serving) ph_flush(a, ph, ph_start, lane);
#endif

    // one atomic per wave for the ray counter
    const unsigned long long total = wave_rays;
    if (lane == 0 && total) atomicAdd(a.ray_counter, total);
    if constexpr (T::ADAPTIVE) {  // ... and one for the samples taken
        if (lane == 0 && wave_samples) atomicAdd(a.ray_counter + 2, wave_samples);
    }
}

#if RT_STRICT && RT_GROUP == 0 && !RT_ADAPT && !RT_FEATURES
// Rank the tiles by probed cost, heaviest first.  A pixel's samples are sequential (one RNG stream), so the frame can
// never end before its longest pixel does: those pixels have to start first, not wherever row-major order puts them.
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t *cost, uint32_t *order, uint32_t n, uint32_t flat_x8)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t peak;
    __shared__ unsigned long long total;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        peak = 1;
        total = 0;
    }
    __syncthreads();
    uint32_t mx = 0;
    unsigned long long sum = 0;
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {
        mx = cost[k] > mx ? cost[k] : mx;
        sum += cost[k];
    }
    atomicMax(&peak, mx);
    atomicAdd(&total, sum);
    __syncthreads();
    const uint32_t top = peak;
    // Nothing to gain where no tile stands out: keep the row-major order.  flat_x8 / 8 = how far the heaviest tile must be above
    // the mean for the order to matter (launcher's choice: 4 where only the longest chains count, less where the spread of
    // ordinary tiles decides the last generation of pixels, see rt_render_launch).
    if ((unsigned long long)top * n * 8ull <= (unsigned long long)flat_x8 * total) {
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) order[k] = k;
        return;
    }
    auto klass = [top](uint32_t c) { return 255u - (uint32_t)(((unsigned long long)c * 255ull) / top); };  // 0 = heaviest
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) atomicAdd(&hist[klass(cost[k])], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int b = 0; b < 256; b++) {
            uint32_t c = hist[b];
            hist[b] = run;
            run += c;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) order[atomicAdd(&hist[klass(cost[k])], 1u)] = k;
}

__global__ __launch_bounds__(256) void classify_pixels_kernel(const uint32_t *cost, uint32_t n, uint32_t threshold, uint8_t *klass,
                                                               uint32_t *list, uint32_t *count, uint32_t *super_list, uint32_t super_threshold,
                                                               uint32_t width, uint32_t near_percent, uint32_t near_neighbours)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    bool heavy = cost[k] >= threshold;
    // The rehearsal is a handful of samples of a heavy-tailed count: a pixel a little under the threshold whose neighbours are over
    // it is more likely a long chain that looked short than a short one (long chains come in patches -- a glass sphere) and goes on
    // the list with them.  A pixel wrongly left with the light ones runs at their pace to the frame's very end.
    if (!heavy && near_neighbours > 0 && width > 0 && cost[k] * 100u >= threshold * near_percent) {
        const uint32_t row = k / width, column = k % width, rows = n / width;
        uint32_t over = 0;
        for (int dr = -1; dr <= 1; dr++)
            for (int dc = -1; dc <= 1; dc++) {
                const int r = (int)row + dr, c = (int)column + dc;
                if ((dr || dc) && r >= 0 && c >= 0 && r < (int)rows && c < (int)width) over += cost[(uint32_t)r * width + (uint32_t)c] >= threshold ? 1u : 0u;
            }
        heavy = over >= near_neighbours;
    }
    const bool longest = heavy && super_list && cost[k] >= super_threshold;
    klass[k] = heavy ? 1 : 0;
    if (longest) super_list[atomicAdd(count + 1, 1u)] = k;
    else if (heavy) list[atomicAdd(count, 1u)] = k;  // order within the list is irrelevant: every listed pixel starts at once
}

hipError_t launch_classify_pixels(const uint32_t *pix_cost, uint32_t n_pixels, uint32_t threshold, uint8_t *pix_class, uint32_t *list,
                                  uint32_t *count, hipStream_t stream, uint32_t *super_list, uint32_t super_threshold, uint32_t width,
                                  uint32_t near_percent, uint32_t near_neighbours)
{
    if (n_pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(classify_pixels_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, pix_cost, n_pixels, threshold,
                       pix_class, list, count, super_list, super_threshold, width, near_percent, near_neighbours);
    return hipGetLastError();
}

// The camera rays' candidate lists (primary_cull_rule.h has the rule and its proof): one thread per 8x8 tile of the rank's rows,
// every thread on the same sphere row at the same time, so the rows come through the scalar path.  The list is written whole, as
// two 16-byte stores; a tile with more than kPrimaryListMax candidates gets "no list".
__global__ __launch_bounds__(256) void primary_lists_kernel(DeviceScene sc, uint16_t *lists, uint32_t n_tiles, int32_t width, int32_t height,
                                                             int32_t rows_owned, int32_t stripe_rows, int32_t rank, int32_t world_size)
{
    const uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= n_tiles) return;
    const CameraRec cam = *sc.camera;
    const TileCone cone = primary_tile_cone(cam, width, height, primary_tile_pixels(tile, width, rows_owned, stripe_rows, rank, world_size));
    uint32_t w[kPrimaryListWords / 2] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // two uint16 per word, the count in the low half of w[0]
    uint32_t count = 0;
    const uint32_t n = sc.n_spheres;
    for (uint32_t s = 0; s < n; s++) {
        const SphereGeom g = load_sphere_row(sc.spheres, s);
        if (!primary_may_hit(cone, g.cx, g.cy, g.cz, g.r2)) continue;
        if (count < kPrimaryListMax) {
            const uint32_t slot = count + 1u;
#pragma unroll
            for (uint32_t q = 0; q < kPrimaryListWords / 2; q++)  // (constant indices: the words stay in registers)
                if (q == slot / 2u) w[q] |= s << ((slot & 1u) * 16u);
        }
        count++;
    }
    if (count > kPrimaryListMax) {
#pragma unroll
        for (uint32_t q = 0; q < kPrimaryListWords / 2; q++) w[q] = 0u;
        count = kPrimaryNoList;
    }
    w[0] |= count;
    uint4 *out = reinterpret_cast<uint4 *>(lists + (size_t)tile * kPrimaryListWords);
    out[0] = uint4{w[0], w[1], w[2], w[3]};
    out[1] = uint4{w[4], w[5], w[6], w[7]};
}

hipError_t launch_primary_lists(const DeviceScene &sc, uint16_t *lists, uint32_t n_tiles, int32_t width, int32_t height, int32_t rows_owned,
                                int32_t stripe_rows, int32_t rank, int32_t world_size, hipStream_t stream)
{
    if (n_tiles == 0) return hipSuccess;
    if (sc.n_spheres > 0xFFFFu) return hipErrorInvalidValue;  // a list entry is a uint16 (the caller builds no lists for such a world)
    hipLaunchKernelGGL(primary_lists_kernel, dim3((n_tiles + 255u) / 256u), dim3(256), 0, stream, sc, lists, n_tiles, width, height, rows_owned,
                       stripe_rows, rank, world_size);
    return hipGetLastError();
}

hipError_t launch_tile_order(const uint32_t *tile_cost, uint32_t *tile_order, uint32_t n_tiles, uint32_t flat_x8, hipStream_t stream)
{
    if (n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, stream, tile_cost, tile_order, n_tiles, flat_x8);
    return hipGetLastError();
}
#endif

#define RT_CAT2(a, b) a##b
#define RT_CAT(a, b) RT_CAT2(a, b)
#if RT_STRICT
#define RT_BUILD strict
#else
#define RT_BUILD fast
#endif
// A scene with a general affine step in some chain (SCENE_AFFINE) is served by the units compiled with RT_AFFINE: every launcher of a
// kernel that walks chains hands such a scene to its twin there, so a scene without one runs the code it ran before.
// A scene with a moving step (SCENE_MOVING) goes one launcher further, to the second pass of the affine unit (RT_MOVING).
#if RT_AFFINE && RT_MOVING
#undef RT_SUFFIX
#undef RT_TO_AFFINE
#define RT_SUFFIX RT_CAT(RT_BUILD, _xm)
#define RT_TO_AFFINE(name, ...) do { } while (0)
#elif RT_AFFINE
#define RT_SUFFIX RT_CAT(RT_BUILD, _x)
#define RT_XM(name) moving::RT_CAT(RT_CAT(name, RT_BUILD), _xm)
#define RT_TO_AFFINE(name, ...) do { if (sc.flags & SCENE_MOVING) return RT_XM(name)(__VA_ARGS__); } while (0)
namespace moving {
hipError_t RT_CAT(RT_CAT(launch_composite_, RT_BUILD), _xm)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_adaptive_composite_, RT_BUILD), _xm)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_features_, RT_BUILD), _xm)(const DeviceScene &sc, const FeatureArgs &a, hipStream_t stream);
hipError_t RT_CAT(RT_CAT(launch_query_, RT_BUILD), _xm)(const DeviceScene &sc, const QueryArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_radiance_, RT_BUILD), _xm)(const DeviceScene &sc, const RadianceArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_step_, RT_BUILD), _xm)(const DeviceScene &sc, const StepArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_advance_, RT_BUILD), _xm)(const DeviceScene &sc, const AdvanceArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_advance_direct_, RT_BUILD), _xm)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_advance_shadow_, RT_BUILD), _xm)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_radiance_direct_, RT_BUILD), _xm)(const DeviceScene &sc, const RadianceDirectArgs &d, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_CAT(RT_CAT(launch_film_direct_, RT_BUILD), _xm)(const DeviceScene &sc, const FilmDirectArgs &d, hipStream_t stream, FilmDirectInfo *info);
}  // namespace moving
#else
#define RT_SUFFIX RT_BUILD
#define RT_X(name) RT_CAT(RT_CAT(name, RT_BUILD), _x)
#define RT_TO_AFFINE(name, ...) do { if (sc.flags & SCENE_AFFINE) return RT_X(name)(__VA_ARGS__); } while (0)
hipError_t RT_X(launch_composite_)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_X(launch_adaptive_composite_)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_X(launch_features_)(const DeviceScene &sc, const FeatureArgs &a, hipStream_t stream);
hipError_t RT_X(launch_query_)(const DeviceScene &sc, const QueryArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_radiance_)(const DeviceScene &sc, const RadianceArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_step_)(const DeviceScene &sc, const StepArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_advance_)(const DeviceScene &sc, const AdvanceArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_advance_direct_)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_advance_shadow_)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_radiance_direct_)(const DeviceScene &sc, const RadianceDirectArgs &d, hipStream_t stream, QueryKernelInfo *info);
hipError_t RT_X(launch_film_direct_)(const DeviceScene &sc, const FilmDirectArgs &d, hipStream_t stream, FilmDirectInfo *info);
#endif

#if RT_GROUP == 0 && !RT_ADAPT && !RT_FEATURES
hipError_t RT_CAT(launch_seed_, RT_SUFFIX)(const SeedArgs &a, hipStream_t stream)
{
    if (a.n_pixels == 0) return hipSuccess;
    dim3 grid((a.n_pixels + 255u) / 256u), block(256);
    hipLaunchKernelGGL(seed_kernel<RT_STRICT>, grid, block, 0, stream, a);
    return hipGetLastError();
}
#endif

namespace {
using TSphereList = Traits<2, false, false, 3>;  // three workgroups per CU serve the heavy and the light pixels (rt_render_launch): 168 VGPRs at most
using TBvhPrims = Traits<0, false, false, 3>;
using TBvhPrimsFast = Traits<0, false, false, 3, false, false, false, 768, true>;  // through the library's own tree
using TBvhGeneral = Traits<0, true, true, 2>;
using TListGeneral = Traits<1, true, true, 2>;
// instances / boxes, no media, plain textures (C4).  168 VGPRs: the instances kernel sits right at the step from three waves per
// SIMD to two
using TBvhInstances = Traits<0, true, false, 3, false>;
// The media and general kernels need ~220 and ~300 VGPRs.  Walking a deep tree they are latency-bound -- one wave per
// SIMD runs at half the speed of two -- so three waves with a hundred-odd registers spilled to scratch still win
// (Cornell smoke +5 %, C5 +4.5 %).  A shallow world with expensive shading (Perlin, image texture) loses a third that
// way, so the general kernel exists in both shapes and the launcher picks by the depth of the world's tree.
using TBvhMedia = Traits<0, true, false, 3, true>;  // + ConstantMedium (Cornell smoke)
using TBvhGeneralDeep = Traits<0, true, true, 3, true, true, false, 768>;
// ... and walked through the library's tree, one walk per run of surface leaves between two media (Traits::SEG): worlds that
// flat_scene.h SCENE_SEGMENTED describes (C5)
using TBvhSegmented = Traits<0, true, true, 3, true, true, false, 768, true>;
// List scans over primitives / instances without media or table-walking textures.  Also the BVH worlds of small
// scenes: for up to 16 leaves within a cost budget (FlatScene::scan_cost) a scan of all of them in the tree's leaf order -- every lane on the same leaf, rows
// through uniform loads, no node visits, no phases -- beats walking the tree (Cornell box: 8 leaves, 7 nodes).  Without
// media no leaf draws random numbers, and as long as every hit lies inside its leaf's box (a moving sphere leaves its box at
// ray times outside its own interval: the launcher then walks, launch_plan.cpp hits_stay_in_boxes), the closest hit is the
// one the walk finds (the reference's own BVH = list invariant; `tests/test_parity_gpu.py::test_small_world_scan_equals_the_bvh_walk`).
// General nesting (REF_TREE leaves, tree_hit): the general kernels plus the interpreter.  Its stack of 16 frames lives in
// scratch -- the reference's own recursion needs a 32 KiB stack per thread (R/kernel.cu:599) -- so these instantiations
// are only ever launched for scenes that nest objects beyond what ObjectRec expresses (none of the ten built-in scenes).
using TBvhNested = Traits<0, true, true, 2, true, false, true>;
using TListNested = Traits<1, true, true, 2, true, false, true>;
using TListPrims = Traits<1, false, false, 4>;  // 127-129 VGPRs without the bound: the strict build would drop to three waves for one register
// 128 VGPRs and 52 B of scratch for a fourth wave per SIMD: C4 +2.4 % (139 VGPRs, none, three waves before)
using TListInstances = Traits<1, true, false, 4, false>;
// The same kernel compiled for FIVE waves per SIMD (96 VGPRs and 64 B of scratch with the path state parked in LDS, Traits::PARK).  Its passes take 1.38 times as long
// -- the SIMDs' issue slots are nearly full with four waves -- so in the steady state it is the slower of the two; but a pixel's
// samples are one chain, pixels of these worlds all cost about the same, and a frame is therefore a whole number of pixel
// "generations" on the resident lanes: 800 x 800 pixels are 2.44 generations on the 262 144 lanes of four waves per SIMD -- three,
// the last 44 % full -- and 1.95 on the 327 680 of five: two.  launch_plan.cpp choose_kernel picks by that count (list_instances_waves).
using TListInstances5 = Traits<1, true, false, 5, false>;
// The same two with the leaves of every ray dealt to lanes (pixels_per_wave < 64: fewer pixels than lanes, the frame is bound
// by the latency of a ray, not by throughput -- registers matter more than a fourth wave)
using TListPrimsGrouped = Traits<1, false, false, 3, false, false, false, 256, false, true>;
using TListInstancesGrouped = Traits<1, true, false, 3, false, false, false, 256, false, true>;

// The host-only planner (launch_plan.h) describes these instantiations by a table of its own: the two must agree.
template <class T>
constexpr KernelProps props_of()
{
    return KernelProps{T::WORLD, T::COMPOSITE, T::RICH, T::MEDIA, T::BATCH, T::NESTED, T::BLOCK, T::FAST, T::SEG, T::GROUPED, T::PARK, T::MIN_WAVES};
}
#define RT_SAME_KERNEL(ID, T) static_assert(same_props(kKernelProps[ID], props_of<T>()), "launch_plan.h kKernelProps[" #ID "] is not " #T)
RT_SAME_KERNEL(K_SPHERE_LIST, TSphereList); RT_SAME_KERNEL(K_BVH_PRIMS, TBvhPrims); RT_SAME_KERNEL(K_BVH_PRIMS_FAST, TBvhPrimsFast);
RT_SAME_KERNEL(K_LIST_PRIMS, TListPrims); RT_SAME_KERNEL(K_LIST_INSTANCES, TListInstances); RT_SAME_KERNEL(K_LIST_INSTANCES_5, TListInstances5);
RT_SAME_KERNEL(K_LIST_PRIMS_GROUPED, TListPrimsGrouped); RT_SAME_KERNEL(K_LIST_INSTANCES_GROUPED, TListInstancesGrouped);
RT_SAME_KERNEL(K_LIST_GENERAL, TListGeneral); RT_SAME_KERNEL(K_LIST_NESTED, TListNested); RT_SAME_KERNEL(K_BVH_INSTANCES, TBvhInstances);
RT_SAME_KERNEL(K_BVH_MEDIA, TBvhMedia); RT_SAME_KERNEL(K_BVH_GENERAL, TBvhGeneral); RT_SAME_KERNEL(K_BVH_GENERAL_DEEP, TBvhGeneralDeep);
RT_SAME_KERNEL(K_BVH_SEGMENTED, TBvhSegmented); RT_SAME_KERNEL(K_BVH_NESTED, TBvhNested);
static_assert(kBigBlock == kBigBlockThreads && kLdsNodeBytes == kStagedNodeBytes && kFastNodeBytes == sizeof(FastNodeF) &&
                  kQueueCap * 64 * sizeof(uint16_t) == kSurvivorQueueBytesPerWave && kParkBytesPerThread == kParkedBytesPerThread,
              "launch_plan.h lays the LDS out with other sizes than the kernels read it with");

// One instantiation, as planned: the LDS layout is lds_layout's (the planner chose T because it fits), the grid is persistent.
template <class T>
hipError_t launch_one(const DeviceScene &sc_in, RenderArgs a, hipStream_t stream, KernelInfo *info)
{
    if (!T::ROLES && a.heavy_list) return hipErrorInvalidValue;  // this instantiation has no serving waves (Traits::ROLES): its listed pixels would never be rendered
    if (T::ADAPTIVE != (a.adaptive != 0) || (T::ADAPTIVE && (a.probe || !a.ad_n || !a.ad_q || !a.ad_mark))) return hipErrorInvalidValue;  // rehearsals run the plain kernels
    // a rehearsal that keeps its samples needs the sum plane; a frame launch behind a capped one, the costs the cap left
    if ((a.probe == 2 && !a.accum) || (a.resumed_spp > 0 && (T::ADAPTIVE || a.probe || !a.accum || (a.probe_ray_cap > 0 && !a.pix_cost)))) return hipErrorInvalidValue;
    auto kernel = render_kernel<RT_STRICT, T>;
    uint32_t tiles = (((uint32_t)a.width + 7u) >> 3) * (((uint32_t)a.rows_owned + 7u) >> 3);
    constexpr KernelProps props = props_of<T>();
    const LdsLayout layout = lds_layout(props, sc_in);
    if (!layout.fits) return hipErrorInvalidValue;  // choose_kernel picks an instantiation that reads its tables from LDS only where they fit
    DeviceScene sc = sc_in;
    apply_layout(layout, sc);
    a.lds_nodes = layout.lds_nodes;
    a.lds_spheres = layout.lds_spheres;
    const size_t lds = layout.bytes;
    if (info) {
        hipFuncAttributes attr;
        hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel));
        if (e != hipSuccess) return e;
        info->vgprs = attr.numRegs;
        info->lds_bytes = (int)(attr.sharedSizeBytes + lds);
        info->kind = kernel_kind(props, T::ADAPTIVE);
        return hipSuccess;
    }
    if (a.n_pixels == 0 || a.spp <= 0) return hipSuccess;
    // persistent grid: as many workgroups as the chip holds at once (never more than there are tiles)
    int per_cu = 0;
    if (lds > kDefaultDynamicLds) {  // more dynamic LDS than the default limit: ask for it (up to the CU's 160 KB)
        hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, T::BLOCK, lds);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    if (a.max_blocks_per_cu > 0 && per_cu > a.max_blocks_per_cu) per_cu = a.max_blocks_per_cu;  // (plan_frame: sphere lists)
    uint32_t resident = (uint32_t)per_cu * (uint32_t)(a.num_cus > 0 ? a.num_cus : 256);
    constexpr uint32_t kWavesPerBlock = (uint32_t)T::BLOCK / 64u;
    uint32_t blocks = (tiles + kWavesPerBlock - 1u) / kWavesPerBlock;
    if (blocks > resident) blocks = resident;
    dim3 grid(blocks), block(T::BLOCK);
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, sc, a);
    return hipGetLastError();
}

} // namespace

// From the planner's kernel id (launch_plan.h KernelId) to its instantiation.  The ids of group 1 are served by the
// RT_GROUP == 1 translation unit, the Adaptive<> forms of both groups by translation units of their own (RT_ADAPT == 1).
hipError_t RT_CAT(launch_composite_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_CAT(launch_adaptive_prims_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);
hipError_t RT_CAT(launch_adaptive_composite_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info);

#if RT_LANE_UNIT
// ------------------------------------------------------------------------------------------------
// Shared by the six lane-per-ray sections below (first-hit features, ray queries, radiance queries, path steps, path advances, light
// sampling): one lane per pixel or per caller-supplied ray or point, no persistent waves; only the light kernels stage anything in
// LDS (their own table).  The next kernel of this family starts from these.
// ------------------------------------------------------------------------------------------------
namespace {
// every table from global memory: a kernel of this family calls this first
DEV void global_tables_only(DeviceScene &sc)
{
    sc.lds_quad_aa = sc.lds_boxes = sc.lds_objects = sc.lds_xforms = sc.lds_media = sc.lds_materials = sc.lds_perlin = kNone;
    sc.lds_spheres_tab = sc.lds_group_boxes = sc.lds_mspheres = sc.lds_msphere_aux = sc.lds_sphere_aux = kNone;
}

// ray k of a caller's arrays, at time[k] or, without that array, at time_all (the feature pass makes its rays itself)
[[maybe_unused]] DEV Ray caller_ray(const double *origin, const double *direction, const double *time, double time_all, uint32_t k)
{
    Ray r;
    r.o = mk(origin[(size_t)k * 3 + 0], origin[(size_t)k * 3 + 1], origin[(size_t)k * 3 + 2]);
    r.d = mk(direction[(size_t)k * 3 + 0], direction[(size_t)k * 3 + 1], direction[(size_t)k * 3 + 2]);
    r.tm = time ? time[k] : time_all;
    return r;
}

// the albedo of a first hit (rt_film_render_features, and rt_scene_intersect after it)
template <class T>
DEV Vec first_hit_albedo(const DeviceScene &sc, const MatView &mp, uint32_t kind, const Surface &s)
{
    if (kind == MAT_METAL) return mp.vec(MAT_OFF(r));
    if (kind == MAT_DIELECTRIC) return mk(1.0, 1.0, 1.0);
    return material_texture<T>(sc, mp, mp.u32(MAT_OFF(tex_inline)), s.u, s.v, s.p);  // Lambertian, isotropic, diffuse light
}

[[maybe_unused]] DEV void store3(double *out, size_t k, Vec v)
{
    out[k * 3 + 0] = v.x;
    out[k * 3 + 1] = v.y;
    out[k * 3 + 2] = v.z;
}

// A stream's six words {d, v0..v4}, `stride` words apart: 1 in the rows rt_rng_state writes (count x 6), n_pixels in a film's planes.
[[maybe_unused]] DEV Xorwow load_stream(const uint32_t *w, size_t stride)
{
    Xorwow rng;
    rng.d = w[0]; rng.v0 = w[stride]; rng.v1 = w[2 * stride]; rng.v2 = w[3 * stride]; rng.v3 = w[4 * stride]; rng.v4 = w[5 * stride];
    return rng;
}
// (the words may be the ones the stream came from: a lane stores only after it has read its six)
[[maybe_unused]] DEV void store_stream(uint32_t *w, size_t stride, const Xorwow &rng)
{
    w[0] = rng.d; w[stride] = rng.v0; w[2 * stride] = rng.v1; w[3 * stride] = rng.v2; w[4 * stride] = rng.v3; w[5 * stride] = rng.v4;
}
// the stream of lane k of a call: row k of rng_in or, without that array, curand_init(seed, k + first_sequence, 0)
template <class Args>
DEV Xorwow lane_stream(const Args &a, uint32_t k)
{
    if (a.rng_in) return load_stream(a.rng_in + (size_t)k * 6, 1);
    Xorwow rng = a.base;
    xorwow_skip_sequences(a.jump_table, a.first_sequence + (uint64_t)k, rng);
    return rng;
}

// The two searches of this family, both the general kernels' search under RT_FLAG_REFERENCE_TREE | RT_FLAG_FORCE_GENERAL: the
// reference's tree (walk_node / walk_leaves) or list (world_hit_list) in the reference's order, never the library's own tree.
//   The closest hit over (0.001, DBL_MAX), what RayColor asks of the world (R/kernel.cu:77), for a kernel that needs the hit
//   record and nothing else: the block "HitInfo h; ... walk_begin<false>(w, ray, DBL_MAX) ... world_hit_list" that feature_kernel,
//   radiance_kernel, step_kernel, advance_kernel and advance_direct_kernel each hold in their own text.  It is not a function
//   because it was measured as one (closest_hit<T>(sc, ray, h, rng), profiles/r30_lane_units_ab.txt): behind the call the tree
//   walk of each kernel compiled with 6 to 14 more SGPRs spilled to VGPR lanes -- the walk_* functions are then first met inside
//   a helper, and the inliner takes them in another order; no way of writing the function changed that -- and radiance_kernel,
//   advance_kernel, advance_direct_kernel and step_kernel ran 6.2 %, 2.5 %, 2.7 % and 1.5 % slower on tree worlds, beyond the
//   spread of the runs; as text they run as before.  A change to one of the five is a change to all.
//   query_search (below, in the units that use it): the caller's interval, the position of the winning leaf from node_leaf_pos
//   and an exit at the first accepted hit -- query_kernel, shadow_kernel, and radiance_direct_kernel and film_direct_kernel, whose
//   one search an iteration is of a path ray or of a shadow ray.  It restates the two short outer loops to note the leaf; the
//   kernels above do not pay for that.
// Termination for any ray, degenerate ones included: the list loop runs n_world_items times; every walk_node step either moves
// to a node with a higher index (n + 1, or an escape link, which always points forward in the preorder array) or parks, a
// parked lane leaves through the escape link, and the last escape is kNone -- at most two steps per node whatever the box tests
// answer (NaNs only make them false); leaf tests are straight-line code or loops over table counts (tree_hit: a bounded stack).
//
// One bounce of RayColor (R/kernel.cu:74-94) behind a search that answered `hit` with record h, exactly the block of render_kernel
// at "R/kernel.cu:74-79": a miss adds the background -- or, under SCENE_ENVIRONMENT, the environment along the ray (miss_value: every
// lane-per-ray kernel gets the environment from this one place) --, a hit goes through make_surface and shade.  Returns scattered: `ray` is then
// the next ray, else it is untouched.  radiance_kernel passes its path's throughput and sum.  Every other caller passes (1, 1, 1)
// and (0, 0, 0): what shade leaves in `accumulated` is then 0 + 1 * x, the emitted or background value x itself, and what it
// leaves in `throughput` is 1 * a, the attenuation a itself (a negative zero comes out positive), in the strict build and in the
// fast one (fma(1, x, 0) is x) -- so a caller that folds acc = acc + thr * emitted, thr = thr * attenuation over the bounces
// repeats radiance_kernel's arithmetic in the strict build.  (A metal whose direction falls below the surface ends the path
// before shade multiplies: throughput is still (1, 1, 1).)  The hit record's facts are query_kernel's: the shading normal where
// want_normal, left (0, 0, 0) for a medium and washed through 0 + n so that no negative zero leaves; the kind where want_kind,
// else 255.  Straight-line code; the rejection loops of shade depend on the stream alone.
template <class T>
DEV bool bounce(const DeviceScene &sc, Ray &ray, const HitInfo &h, bool hit, Xorwow &rng, Vec &throughput, Vec &accumulated, bool want_normal,
                bool want_kind, Vec &normal, bool &front, uint32_t &kind)
{
    normal = mk(0.0, 0.0, 0.0);
    kind = 255u;
    front = false;
    bool scattered = false;
    if (!hit) {  // R/kernel.cu:74-79
        accumulated = accumulated + throughput * miss_value<T>(sc, sc.camera, ray.d);
    } else {
        const Surface s = make_surface<T>(sc, ray, h);
        if (want_normal && (h.ref >> kRefShift) != REF_MEDIUM) normal = s.n;
        front = s.front;
        if (want_kind) kind = material_view<false>(sc, s.mat).u32(MAT_OFF(kind));
        scattered = shade<T>(sc, s, ray, throughput, accumulated, rng);
    }
    normal = mk(0.0, 0.0, 0.0) + normal;
    return scattered;
}
// (a caller that wants none of the hit record's facts)
template <class T>
DEV bool bounce(const DeviceScene &sc, Ray &ray, const HitInfo &h, bool hit, Xorwow &rng, Vec &throughput, Vec &accumulated)
{
    Vec normal;
    bool front;
    uint32_t kind;
    return bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, false, false, normal, front, kind);
}

// What the scan and the gather behind a path advance read: row k's survivor flag and the workgroup's count of survivors -- per
// wave, then one store (as count_valid reduces) -- and one atomic per wave for the rows that took a step.  Every lane of the
// workgroup comes here, rows at or beyond the count and dead rays as non-survivors.
[[maybe_unused]] DEV void count_survivors(const AdvanceArgs &a, uint32_t k, bool stepped, bool scattered, uint32_t *wave_survivors)
{
    if (k < a.capacity) a.survivor[k] = scattered ? 1 : 0;
    const unsigned long long survivors = __ballot(scattered);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_survivors[wave] = (uint32_t)__popcll(survivors);
    if (a.stepped_counter) {
        const unsigned long long took = __ballot(stepped);
        if (lane == 0 && took) atomicAdd(a.stepped_counter, (unsigned long long)__popcll(took));
    }
    __syncthreads();
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = (wave_survivors[0] + wave_survivors[1]) + (wave_survivors[2] + wave_survivors[3]);
}

// info != nullptr: report the registers and scratch of the chosen instantiation instead of launching it; else a lane per ray
template <class Args>
hipError_t info_or_launch(void (*kernel)(DeviceScene, Args), const DeviceScene &sc, const Args &a, uint32_t count, hipStream_t stream, QueryKernelInfo *info)
{
    if (info) {
        hipFuncAttributes attr;
        if (hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel)); e != hipSuccess) return e;
        info->vgprs = attr.numRegs;
        info->scratch_bytes = (int)attr.localSizeBytes;
        return hipSuccess;
    }
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, sc, a);
    return hipGetLastError();
}
}  // namespace
#endif

#if RT_FEATURES
// ------------------------------------------------------------------------------------------------
// First-hit feature pass (rt_film_render_features): albedo, shading normal and depth of the closest hit over [0.001, inf) of
// every primary ray.  One lane per owned pixel, no persistent waves, no LDS staging, every table from global memory; the search
// is the closest-hit block (the comment on the two searches above), so that media draw what they draw in a render and coincident primitives are decided as the reference decides
// them, and the hit record is make_surface's.
// ------------------------------------------------------------------------------------------------
namespace {
// samples == 0: the ray through the pixel centre, no lens offset, at the shutter's opening; the camera takes no draws
DEV Ray centre_ray(const CameraRec *cam_generic, int i, int j, int width, int height)
{
    const RT_CONST CameraRec *cam = (const RT_CONST CameraRec *)(uintptr_t)cam_generic;
    const double u = ((double)i + 0.5) / (double)width, v = ((double)j + 0.5) / (double)height;
    const Vec origin = load3c(cam->origin);
    Ray r;
    r.o = origin;
    r.d = load3c(cam->llc) + u * load3c(cam->horizontal) + v * load3c(cam->vertical) - origin;
    r.tm = cam->time0;
    return r;
}
}  // namespace

template <int STRICT, class T>
__global__ __launch_bounds__(256) void feature_kernel(DeviceScene sc, FeatureArgs a)
{
    global_tables_only(sc);
    const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= a.n_pixels) return;
    const int lr = (int)(local / (uint32_t)a.width), i = (int)(local % (uint32_t)a.width);
    const int j = owned_row(lr, a.stripe_rows, a.rank, a.world_size);
    Xorwow rng = a.base;  // as seed_kernel seeds the pixel: pixelIndex, R/kernel.cu:117-118
    xorwow_skip_sequences(a.jump_table, (uint64_t)((int64_t)j * a.width + i), rng);
    const CameraRec *__restrict__ cam = sc.camera;
    const NodeView nv{sc.nodes, 0u, false};
    Vec albedo = mk(0.0, 0.0, 0.0), normal = mk(0.0, 0.0, 0.0);
    double depth = 0.0;
    const int n = a.samples > 0 ? a.samples : 1;
    for (int sample = 0; sample < n; sample++) {
        const Ray ray = a.samples > 0 ? camera_ray(cam, i, j, a.width, a.height, rng) : centre_ray(cam, i, j, a.width, a.height);
        HitInfo h;
        h.t = 0.0;
        h.ref = kNone;
        h.obj = kNone;
        bool hit = false;
        if constexpr (T::WORLD == 0) {
            if (sc.n_world_nodes != 0) {
                Walk w{};
                walk_begin<false>(w, ray, DBL_MAX);
                while (w.state != kNone) {
                    if (walk_moving(w.state)) walk_node<false>(nv, ray, 0.001, w);
                    else walk_leaves<T>(sc, nv, ray, 0.001, w, h, rng);
                }
                hit = w.any;
            }
        } else {
            hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng);
        }
        Vec value, sn = mk(0.0, 0.0, 0.0);
        double sd = 0.0;
        if (!hit) {
            value = miss_value<T>(sc, cam, ray.d);
        } else {
            const Surface s = make_surface<T>(sc, ray, h);
            const MatView mp = material_view<false>(sc, s.mat);
            value = first_hit_albedo<T>(sc, mp, mp.u32(MAT_OFF(kind)), s);
            if ((h.ref >> kRefShift) != REF_MEDIUM) sn = s.n;
            sd = h.t * length(ray.d);
        }
        // the sum as a render forms it: accumulated = 0 + throughput (1, 1, 1) * value, col += accumulated (render_kernel)
        albedo = albedo + (mk(0.0, 0.0, 0.0) + mk(1.0, 1.0, 1.0) * value);
        normal = normal + sn;
        depth = depth + sd;
    }
    if (a.samples > 0) {
        albedo = over(albedo, (double)n);
        normal = over(normal, (double)n);
        depth = (1 / (double)n) * depth;
    }
    store3(a.albedo, local, albedo);
    store3(a.normal, local, normal);
    a.depth[local] = depth;
}

hipError_t RT_CAT(launch_features_, RT_SUFFIX)(const DeviceScene &sc, const FeatureArgs &a, hipStream_t stream)
{
    RT_TO_AFFINE(launch_features_, sc, a, stream);
    if (a.n_pixels == 0) return hipSuccess;
    const dim3 grid((a.n_pixels + 255u) / 256u), block(256);
    if (sc.world_kind == WORLD_BVH) hipLaunchKernelGGL((feature_kernel<RT_STRICT, TBvhNested>), grid, block, 0, stream, sc, a);
    else hipLaunchKernelGGL((feature_kernel<RT_STRICT, TListNested>), grid, block, 0, stream, sc, a);
    return hipGetLastError();
}
#endif
#if RT_QUERY || RT_ADVANCE_DIRECT || RT_RADIANCE_DIRECT || RT_FILM_DIRECT  // (the search is shadow_kernel's, radiance_direct_kernel's and film_direct_kernel's too)
// ------------------------------------------------------------------------------------------------
// Ray queries (rt_scene_intersect): closest hit or occlusion for caller-supplied rays.  One lane per ray, no LDS, every table from
// global memory, the ray, its time and its interval read from the caller's arrays.  query_search is the closest-hit search (the
// comment on the two searches above says which kernel uses which, and why it terminates) over this section's copies of the two short outer loops
// (world_hit_list, walk_leaves), which note the world leaf that produced the winning record and, for an occlusion query of a
// world without media, stop at the first accepted hit.  The library's own tree is never walked here: valid only while hits stay
// inside their leaves' boxes, which depends on the shutter; a caller's times are arbitrary.
// ------------------------------------------------------------------------------------------------
namespace {
// R/HittableList.h:39-57 as world_hit_list runs it, plus the position of the winning leaf; FIRST: leave at the first accepted hit
template <class T>
DEV bool query_hit_list(const DeviceScene &sc, const Ray &r, double tmin, double tmax, bool first, HitInfo &best, uint32_t &leaf, Xorwow &rng)
{
    const double a = dot(r.d, r.d);
    double closest = tmax;
    bool any = false;
    const uint32_t n = sc.n_world_items;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t ref = (uint32_t)__builtin_amdgcn_readfirstlane((int)((const RT_CONST uint32_t *)(uintptr_t)sc.world_items)[k]);
        if (leaf_test<T>(sc, ref, r, a, tmin, closest, best, rng)) {
            any = true;
            closest = best.t;
            leaf = k;
            if (first) break;
        }
    }
    return any;
}

// walk_leaves for a parked lane (the bottom node's one or two leaves in the reference's order; a span-1 node holds its leaf twice and
// only a medium is tested again), plus the position of the winning leaf from the table parallel to nodes[]
template <class T>
DEV void query_walk_leaves(const DeviceScene &sc, const uint32_t *__restrict__ node_leaf_pos, const Ray &r, double tmin, Walk &w, HitInfo &best,
                           uint32_t &leaf, Xorwow &rng)
{
    const uint32_t n = w.state & ~kWalkParked;
    const BvhNodeRec *node = sc.nodes + n;
    const uint32_t na = node->a, nb = node->b, next = node->escape;
    const bool again = nb != na || is_medium_leaf(nb);
    for (int c = 0; c < 2; c++) {  // one inlined copy of the leaf test
        if (c == 1 && !again) break;
        if (leaf_test<T>(sc, c ? nb : na, r, w.a, tmin, w.closest, best, rng)) {
            w.any = true;
            w.closest = best.t;
            leaf = node_leaf_pos[2u * n + (uint32_t)c];
        }
    }
    w.state = next;
}

// the search over the two loops above: the position of the winning leaf into `leaf`; first: no more than one accepted hit
template <class T>
DEV bool query_search(const DeviceScene &sc, const uint32_t *node_leaf_pos, const Ray &ray, double tmin, double tmax, bool first, HitInfo &h,
                      uint32_t &leaf, Xorwow &rng)
{
    h.t = 0.0;
    h.ref = kNone;
    h.obj = kNone;
    if constexpr (T::WORLD == 0) {
        if (sc.n_world_nodes == 0) return false;
        const NodeView nv{sc.nodes, 0u, false};
        Walk w{};
        walk_begin<false>(w, ray, tmax);
        while (w.state != kNone) {
            if (walk_moving(w.state)) {
                walk_node<false>(nv, ray, tmin, w);
            } else {
                query_walk_leaves<T>(sc, node_leaf_pos, ray, tmin, w, h, leaf, rng);
                if (first && w.any) break;
            }
        }
        return w.any;
    } else {
        return query_hit_list<T>(sc, ray, tmin, tmax, first, h, leaf, rng);
    }
}

// HitRecord U, V of the primitive that won (R/Sphere.h:44, R/MovingSphere.h:70, R/Quad.h:96-97), in the space the hit was found in
// as make_surface finds it -- which computes them only for materials that read them
template <class T>
DEV void query_uv(const DeviceScene &sc, const Ray &r, const HitInfo &h, double &u, double &v)
{
    u = 0.0;
    v = 0.0;
    const uint32_t tag = h.ref >> kRefShift, idx = h.ref & kRefIndexMask;
    if (tag == REF_MEDIUM) return;
    Ray lr = r;
    if (h.obj != kNone) {
        uint32_t xf_first, xf_count;
        if (h.obj & kTreeObjBit) {
            const TreeNodeRec n = sc.tree_nodes[h.obj & ~kTreeObjBit];
            xf_first = n.chain_first;
            xf_count = n.chain_count;
        } else {
            const ObjectRec o = get_object(sc, h.obj);
            xf_first = o.xf_first;
            xf_count = o.xf_count;
        }
        lr = chain_ray(sc, xf_first, xf_count, r);
    }
    const Vec p = at(lr, h.t);
    if (tag == REF_QUAD) {
        const QuadGeom q = sc.quads[idx];
        const Vec ph = p - mk(q.qx, q.qy, q.qz), w = mk(q.wx, q.wy, q.wz);
        u = dot(w, cross(ph, mk(q.vx, q.vy, q.vz)));
        v = dot(w, cross(mk(q.ux, q.uy, q.uz), ph));
        if (const uint32_t row = attr_row(sc, idx)) {
            const RT_CONST double *a = const_doubles(sc.quads + row);
            if (((const RT_CONST uint32_t *)a)[30] & ATTR_TEXCOORDS) attr_uv(a, u, v, (1.0 - u) - v, u, v);
        }
    } else if (tag == REF_SPHERE) {
        const SphereGeom g = sc.spheres[idx];
        sphere_uv(sc.sphere_aux[idx].inv_r * (p - mk(g.cx, g.cy, g.cz)), u, v);
    } else {
        const Vec c = msphere_center(sc.mspheres[idx], lr.tm, (sc.flags & SCENE_MS_UNIT_TIME) != 0);
        sphere_uv(sc.msphere_aux[idx].inv_r * (p - c), u, v);
    }
}
}  // namespace
#endif

#if RT_QUERY
// MODE 0 closest hit, 1 occlusion
template <int STRICT, class T, int MODE>
__global__ __launch_bounds__(256) void query_kernel(DeviceScene sc, QueryArgs a)
{
    global_tables_only(sc);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.count) return;
    const Ray ray = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
    const double tmin = a.tmin ? a.tmin[k] : a.tmin_all;
    const double tmax = fmin(a.tmax ? a.tmax[k] : a.tmax_all, DBL_MAX);  // +inf: DBL_MAX, what a render passes (R/kernel.cu:77)
    const bool media = (sc.flags & SCENE_HAS_MEDIA) != 0;
    Xorwow rng = a.base;  // curand_init(seed, k + first_sequence, 0); only a medium's test draws
    if (media) xorwow_skip_sequences(a.jump_table, a.first_sequence + (uint64_t)k, rng);
    const bool first = MODE == 1 && !media;  // a medium's answer depends on what was found before it: the full search
    HitInfo h;
    uint32_t leaf = kNone;
    const bool hit = query_search<T>(sc, a.node_leaf_pos, ray, tmin, tmax, first, h, leaf, rng);
    if (a.hit_counter) {
        const unsigned long long found = __ballot(hit);  // one atomic per wave (per group of lanes that arrive together)
        if (hit && (uint32_t)__ffsll((long long)found) - 1u == (threadIdx.x & 63u)) atomicAdd(a.hit_counter, (unsigned long long)__popcll(found));
    }
    if (a.occluded) a.occluded[k] = hit ? 1 : 0;
    if constexpr (MODE == 0) {
        if (a.t) a.t[k] = hit ? h.t : (double)INFINITY;
        if (a.leaf) a.leaf[k] = hit ? (int32_t)leaf : -1;
        const bool want_material = a.material || a.albedo;
        if (!(a.normal || a.uv || a.front_face || want_material)) return;
        Vec normal = mk(0.0, 0.0, 0.0), value = mk(0.0, 0.0, 0.0);
        double u = 0.0, v = 0.0;
        uint32_t kind = 255u;
        bool front = false;
        if (!hit) {
            if (a.albedo) value = miss_value<T>(sc, sc.camera, ray.d);
        } else {
            if (a.uv) query_uv<T>(sc, ray, h, u, v);
            if (a.normal || a.front_face || want_material) {  // (U/V alone need no hit record)
                const Surface s = make_surface<T>(sc, ray, h);
                if ((h.ref >> kRefShift) != REF_MEDIUM) normal = s.n;
                front = s.front;
                if (want_material) {
                    const MatView mp = material_view<false>(sc, s.mat);
                    kind = mp.u32(MAT_OFF(kind));
                    if (a.albedo) value = first_hit_albedo<T>(sc, mp, kind, s);
                }
            }
        }
        // as the feature pass stores its one sample, 0 + x: no negative zeros
        value = mk(0.0, 0.0, 0.0) + (mk(0.0, 0.0, 0.0) + mk(1.0, 1.0, 1.0) * value);
        normal = mk(0.0, 0.0, 0.0) + normal;
        if (a.normal) store3(a.normal, k, normal);
        if (a.uv) {
            a.uv[(size_t)k * 2 + 0] = u;
            a.uv[(size_t)k * 2 + 1] = v;
        }
        if (a.albedo) store3(a.albedo, k, value);
        if (a.front_face) a.front_face[k] = front ? 1 : 0;
        if (a.material) a.material[k] = (uint8_t)kind;
    }
}

hipError_t RT_CAT(launch_query_, RT_SUFFIX)(const DeviceScene &sc, const QueryArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_query_, sc, a, stream, info);
    if (a.mode != 0 && a.mode != 1) return hipErrorInvalidValue;
    if (sc.world_kind == WORLD_BVH && !a.node_leaf_pos) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, QueryArgs);
    if (sc.world_kind == WORLD_BVH) kernel = a.mode == 0 ? query_kernel<RT_STRICT, TBvhNested, 0> : query_kernel<RT_STRICT, TBvhNested, 1>;
    else kernel = a.mode == 0 ? query_kernel<RT_STRICT, TListNested, 0> : query_kernel<RT_STRICT, TListNested, 1>;
    return info_or_launch(kernel, sc, a, a.count, stream, info);
}
#elif RT_RADIANCE
// ------------------------------------------------------------------------------------------------
// Radiance queries (rt_scene_radiance): RayColor (R/kernel.cu:66-98) for caller-supplied rays.  One lane per ray, no LDS, every
// table from global memory; the closest-hit search, then bounce on the path's own
// throughput and sum.
// One flattened loop: an iteration is one world search and one shade step for every lane still live; a lane whose path ends adds
// it to its sum and starts its next sample, from the same ray, in the same iteration (render_kernel's path regeneration), and
// leaves when its last sample is done.  Lanes at different samples and depths so share the search code; a loop over samples
// around a loop over bounces would idle every lane until the longest path of each round ends.
// Termination for any ray: at most samples * max_depth iterations, each a bounded search and a bounce.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T>
__global__ __launch_bounds__(256) void radiance_kernel(DeviceScene sc, RadianceArgs a)
{
    global_tables_only(sc);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rays = 0;  // world searches of this lane's ray, all samples
    if (k < a.count) {
        const Ray first = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
        Xorwow rng = lane_stream(a, k);
        const NodeView nv{sc.nodes, 0u, false};
        Vec sum = mk(0.0, 0.0, 0.0);
        if (a.max_depth > 0) {  // R/kernel.cu:71: otherwise the bounce loop never runs, RayColor returns black and draws nothing
            Ray ray = first;
            Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
            int depth = 0, sample = 0;
            for (;;) {
                HitInfo h;
                h.t = 0.0;
                h.ref = kNone;
                h.obj = kNone;
                bool hit = false;
                if constexpr (T::WORLD == 0) {
                    if (sc.n_world_nodes != 0) {
                        Walk w{};
                        walk_begin<false>(w, ray, DBL_MAX);
                        while (w.state != kNone) {
                            if (walk_moving(w.state)) walk_node<false>(nv, ray, 0.001, w);
                            else walk_leaves<T>(sc, nv, ray, 0.001, w, h, rng);
                        }
                        hit = w.any;
                    }
                } else {
                    hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng);
                }
                rays++;
                bool path_ends = !bounce<T>(sc, ray, h, hit, rng, throughput, accumulated);
                if (!path_ends && ++depth >= a.max_depth) path_ends = true;  // R/kernel.cu:71,97
                if (path_ends) {  // R/kernel.cu:143: col += RayColor(...)
                    sum = sum + accumulated;
                    if (++sample >= a.samples) break;
                    ray = first;
                    throughput = mk(1.0, 1.0, 1.0);
                    accumulated = mk(0.0, 0.0, 0.0);
                    depth = 0;
                }
            }
        }
        if (a.radiance) {  // linear: the mean as a render forms it (R/kernel.cu:150), no gamma
            const Vec mean = over(sum, (double)a.samples);
            store3(a.radiance, k, mean);
        }
        if (a.path_rays) a.path_rays[k] = rays;
        if (a.rng_out) store_stream(a.rng_out + (size_t)k * 6, 1, rng);
    }
    if (a.ray_counter) {  // one atomic per wave: every lane of the wave is here again
        unsigned long long total = rays;
        for (int step = 32; step > 0; step >>= 1) total += __shfl_xor(total, step, 64);
        if ((threadIdx.x & 63u) == 0 && total) atomicAdd(a.ray_counter, total);
    }
}

hipError_t RT_CAT(launch_radiance_, RT_SUFFIX)(const DeviceScene &sc, const RadianceArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_radiance_, sc, a, stream, info);
    if (a.samples < 1 || a.max_depth < 0 || !a.origin || !a.direction || !(a.radiance || a.path_rays || a.rng_out)) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, RadianceArgs) =
        sc.world_kind == WORLD_BVH ? radiance_kernel<RT_STRICT, TBvhNested> : radiance_kernel<RT_STRICT, TListNested>;
    return info_or_launch(kernel, sc, a, a.count, stream, info);
}
#elif RT_STEP
// ------------------------------------------------------------------------------------------------
// Path steps (rt_scene_path_step): one iteration of RayColor's loop (R/kernel.cu:74-94) for caller-supplied rays, so that an
// integrator outside the library can continue the path itself.  radiance_kernel's iteration -- the closest-hit search and bounce -- run once,
// from throughput (1, 1, 1) and accumulated (0, 0, 0), which come back as the attenuation and the emitted or background value
// themselves (bounce says why).  Termination for any ray: one bounded search and one bounce.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T>
__global__ __launch_bounds__(256) void step_kernel(DeviceScene sc, StepArgs a)
{
    global_tables_only(sc);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.count) return;
    // the ray and the six words are read here, before anything is written: every output may be the input array of the same meaning
    Ray ray = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
    Xorwow rng = lane_stream(a, k);
    const NodeView nv{sc.nodes, 0u, false};
    Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
    HitInfo h;
    h.t = 0.0;
    h.ref = kNone;
    h.obj = kNone;
    bool hit = false;
    if constexpr (T::WORLD == 0) {
        if (sc.n_world_nodes != 0) {
            Walk w{};
            walk_begin<false>(w, ray, DBL_MAX);
            while (w.state != kNone) {
                if (walk_moving(w.state)) walk_node<false>(nv, ray, 0.001, w);
                else walk_leaves<T>(sc, nv, ray, 0.001, w, h, rng);
            }
            hit = w.any;
        }
    } else {
        hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng);
    }
    Vec normal;
    uint32_t kind;
    bool front;
    const bool scattered = bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, a.normal != nullptr, a.material != nullptr, normal, front, kind);
    if (a.scattered_counter) {
        const unsigned long long found = __ballot(scattered);  // one atomic per wave (per group of lanes that arrive together)
        if (scattered && (uint32_t)__ffsll((long long)found) - 1u == (threadIdx.x & 63u))
            atomicAdd(a.scattered_counter, (unsigned long long)__popcll(found));
    }
    if (a.status) a.status[k] = !hit ? 0 : scattered ? 2 : 1;
    if (a.emitted) store3(a.emitted, k, accumulated);
    if (a.attenuation) store3(a.attenuation, k, scattered ? throughput : mk(0.0, 0.0, 0.0));
    if (a.origin_out) store3(a.origin_out, k, ray.o);
    if (a.direction_out) store3(a.direction_out, k, ray.d);
    if (a.time_out) a.time_out[k] = ray.tm;
    if (a.t) a.t[k] = hit ? h.t : (double)INFINITY;
    if (a.normal) store3(a.normal, k, normal);
    if (a.front_face) a.front_face[k] = front ? 1 : 0;
    if (a.material) a.material[k] = (uint8_t)kind;
    if (a.rng_out) store_stream(a.rng_out + (size_t)k * 6, 1, rng);
}

hipError_t RT_CAT(launch_step_, RT_SUFFIX)(const DeviceScene &sc, const StepArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_step_, sc, a, stream, info);
    const bool any = a.status || a.emitted || a.attenuation || a.origin_out || a.direction_out || a.time_out || a.t || a.normal || a.front_face ||
                     a.material || a.rng_out;
    if (!a.origin || !a.direction || !any) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, StepArgs) = sc.world_kind == WORLD_BVH ? step_kernel<RT_STRICT, TBvhNested> : step_kernel<RT_STRICT, TListNested>;
    return info_or_launch(kernel, sc, a, a.count, stream, info);
}
#elif RT_ADVANCE
// ------------------------------------------------------------------------------------------------
// Path advances (rt_scene_path_advance), launch 1 of 3 (render_iface.h AdvanceArgs): step_kernel's iteration (the
// closest-hit search and bounce) for every row below n = min(*count_in, capacity) whose ray is alive, and then what a caller's loop did with the outputs:
//   an ended ray (status 0 or 1) adds thr * emitted to its row of `radiance` -- the product, then the sum, two operations in the
//   strict build; the ids of live rays are distinct, so a plain load, add and store;
//   a scattered ray (status 2) stages its record at its own row k of the staging arrays and sets survivor[k]; the gather launch
//   moves it to its packed row once the scan launch knows how many survivors the workgroups before this one have.
// The throughput and the id are loaded after the search: they are not live across it.  No lane returns early: rows at or beyond n
// and dead rays reach count_survivors as non-survivors, and every row below `capacity` gets its flag, every workgroup its count,
// so that the two launches behind this one read nothing stale.  Termination as for step_kernel.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T>
__global__ __launch_bounds__(256) void advance_kernel(DeviceScene sc, AdvanceArgs a)
{
    __shared__ uint32_t wave_survivors[4];
    global_tables_only(sc);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = a.count_in ? min(*a.count_in, a.capacity) : a.capacity;
    const bool stepped = k < n && (!a.alive || a.alive[k] != 0);
    bool scattered = false;
    if (stepped) {
        Ray ray = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
        Xorwow rng = lane_stream(a, k);
        const NodeView nv{sc.nodes, 0u, false};
        Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
        HitInfo h;
        h.t = 0.0;
        h.ref = kNone;
        h.obj = kNone;
        bool hit = false;
        if constexpr (T::WORLD == 0) {
            if (sc.n_world_nodes != 0) {
                Walk w{};
                walk_begin<false>(w, ray, DBL_MAX);
                while (w.state != kNone) {
                    if (walk_moving(w.state)) walk_node<false>(nv, ray, 0.001, w);
                    else walk_leaves<T>(sc, nv, ray, 0.001, w, h, rng);
                }
                hit = w.any;
            }
        } else {
            hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng);
        }
        Vec normal;
        uint32_t kind;
        bool front;
        scattered = bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, a.stage.normal != nullptr, a.stage.material != nullptr, normal, front, kind);
        // what the path carried into this bounce: `throughput` is 1 * attenuation and `accumulated` 0 + 1 * emitted (bounce)
        const Vec carried = a.throughput ? mk(a.throughput[(size_t)k * 3 + 0], a.throughput[(size_t)k * 3 + 1], a.throughput[(size_t)k * 3 + 2])
                                         : mk(1.0, 1.0, 1.0);
        const int32_t id = a.ray_id ? a.ray_id[k] : (int32_t)k;
        if (!scattered) {
            if (a.radiance && id >= 0 && (uint32_t)id < a.sources) {
                const Vec product = carried * accumulated;
                double *row = a.radiance + (size_t)id * 3;
                const Vec sum = mk(row[0], row[1], row[2]) + product;
                row[0] = sum.x;
                row[1] = sum.y;
                row[2] = sum.z;
            }
        } else {
            if (a.stage.origin) store3(a.stage.origin, k, ray.o);
            if (a.stage.direction) store3(a.stage.direction, k, ray.d);
            if (a.stage.time) a.stage.time[k] = ray.tm;
            if (a.stage.rng_state) store_stream(a.stage.rng_state + (size_t)k * 6, 1, rng);
            if (a.stage.throughput) store3(a.stage.throughput, k, carried * throughput);
            if (a.stage.ray_id) a.stage.ray_id[k] = id;
            if (a.stage.t) a.stage.t[k] = h.t;
            if (a.stage.normal) store3(a.stage.normal, k, normal);
            if (a.stage.front_face) a.stage.front_face[k] = front ? 1 : 0;
            if (a.stage.material) a.stage.material[k] = (uint8_t)kind;
        }
    }
    count_survivors(a, k, stepped, scattered, wave_survivors);  // every lane of the workgroup is here again
}

hipError_t RT_CAT(launch_advance_, RT_SUFFIX)(const DeviceScene &sc, const AdvanceArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_advance_, sc, a, stream, info);
    if (!info && (!a.origin || !a.direction || !a.survivor || !a.block_counts)) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, AdvanceArgs) =
        sc.world_kind == WORLD_BVH ? advance_kernel<RT_STRICT, TBvhNested> : advance_kernel<RT_STRICT, TListNested>;
    return info_or_launch(kernel, sc, a, a.capacity, stream, info);
}
#endif
#if RT_LIGHTS || RT_ADVANCE_DIRECT || RT_RADIANCE_DIRECT || RT_FILM_DIRECT  // (the staging and the table's readers are advance_direct_kernel's, radiance_direct_kernel's and film_direct_kernel's too)
// ------------------------------------------------------------------------------------------------
// Light sampling queries (rt_scene_sample_lights, rt_scene_light_pdf; include/rtow.h states both operation by operation, and
// tests/light_restated.py restates the strict build to the bit).  One lane per point or ray, the callers' arrays read and written
// coalesced.  The light table comes through LightArgs, in world space: no object records, no transforms, no search of the world.
// A workgroup first stages the first kLightLdsRows rows and their entries of the call's cumulative table in LDS with 16-byte
// loads; rows beyond the cap come from global memory.  light_sample_kernel reads one row per lane (whichever its draw picked);
// light_pdf_kernel loops over all rows wave-uniformly, every lane on the same row -- an LDS broadcast -- which is the count x
// n_lights loop the staging is for.  No lane returns early (all meet at the barriers), no wave waits for another workgroup; the
// count of valid results reduces per wave, then per workgroup, then one atomic.
// ------------------------------------------------------------------------------------------------
namespace {
constexpr double kLightPi = 3.1415926535897932385;
constexpr uint32_t kLightRowDoubles = (uint32_t)(sizeof(LightRow) / sizeof(double));
static_assert(kLightLdsRows % 2 == 0 && sizeof(LightRow) % 16 == 0, "whole 16-byte loads");

struct LightLds {
    const double *rows, *cdf;  // the workgroup's copies
};
DEV void stage_lights(const LightArgs &a, double *rows_lds, double *cdf_lds)
{
    const uint32_t n = min(a.n_lights, kLightLdsRows);
    const double2 *src = reinterpret_cast<const double2 *>(a.rows);
    double2 *dst = reinterpret_cast<double2 *>(rows_lds);
    for (uint32_t i = threadIdx.x; i < n * (kLightRowDoubles / 2u); i += 256u) dst[i] = src[i];
    // (the table is padded to an even length, and kLightLdsRows is even: the last pair is in bounds on both sides)
    const double2 *csrc = reinterpret_cast<const double2 *>(a.cdf);
    double2 *cdst = reinterpret_cast<double2 *>(cdf_lds);
    for (uint32_t i = threadIdx.x; i < (n + 1u) / 2u; i += 256u) cdst[i] = csrc[i];
    __syncthreads();
}
DEV LightRow light_row(const LightArgs &a, const LightLds &lds, uint32_t i)
{
    if (i < kLightLdsRows) return *reinterpret_cast<const LightRow *>(lds.rows + (size_t)i * kLightRowDoubles);
    return a.rows[i];
}
DEV double light_cdf(const LightArgs &a, const LightLds &lds, uint32_t i) { return i < kLightLdsRows ? lds.cdf[i] : a.cdf[i]; }
DEV Vec load3(const double *p) { return mk(p[0], p[1], p[2]); }
DEV Vec light_centre(const LightRow &L, double tm)  // MSphereGeom's formula for a moving sphere
{
    if (L.kind == LIGHT_MSPHERE) return load3(L.a) + ((tm - L.c[0]) / L.c[1]) * load3(L.b);
    return load3(L.a);
}
DEV bool usable_density(double pdf) { return pdf > 0.0 && pdf < (double)INFINITY; }  // (a NaN is not)
// the valid results of the workgroup: per wave, then one atomic
[[maybe_unused]] DEV void count_valid(unsigned long long *counter, bool valid, uint32_t *wave_valid)  // (the light kernels)
{
    const unsigned long long found = __ballot(valid);
    if ((threadIdx.x & 63u) == 0) wave_valid[threadIdx.x >> 6] = (uint32_t)__popcll(found);
    __syncthreads();
    if (threadIdx.x == 0 && counter) {
        const uint32_t total = (wave_valid[0] + wave_valid[1]) + (wave_valid[2] + wave_valid[3]);
        if (total) atomicAdd(counter, (unsigned long long)total);
    }
}

// The light sample of rt_scene_sample_lights for the point P at the time tm, drawn from rng (include/rtow.h states it operation by
// operation, tests/light_restated.py restates the strict build to the bit; n_lights != 0).  One draw picks the row: `row` is the
// first with cdf >= xi by bisection (the last entry is 1.0 >= xi), L that row.  A parallelogram or triangle takes two draws for
// the point S = a + ua b + ub c (a triangle folds ua + ub > 1 back), (u, v) = (ua, ub).  A sphere takes the rejection loop of the
// lens for a point of the unit disc and maps it into the cone the sphere subtends from P, around the axis to `centre` (a moving
// sphere's centre at tm); `distance` is then the near root as the renderer's own sphere test finds it for this ray (sphere_test /
// sphere_roots: R/Sphere.h:28-50), operation by operation -- a shadow ray along `dir` meets the lamp at this very parameter --
// and S the point there.  Returns validity; an invalid sample leaves dir (0, 0, 0), distance 0 and pdf 0, and has taken the same
// draws.  Termination: the bisection halves hi - lo; the rejection loop depends on the stream alone.
[[maybe_unused]] DEV bool light_sample(const LightArgs &a, const LightLds &lds, Vec P, double tm, Xorwow &rng, uint32_t &row, LightRow &L, Vec &dir,
                                      double &distance, double &pdf, Vec &S, Vec &centre, double &u, double &v)
{
    bool valid = false;
    dir = mk(0.0, 0.0, 0.0);
    distance = 0.0;
    pdf = 0.0;
    const double xi = (double)xorwow_uniform(rng);
    uint32_t lo = 0, hi = a.n_lights - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (light_cdf(a, lds, mid) >= xi) hi = mid;
        else lo = mid + 1u;
    }
    row = lo;
    const double chance = light_cdf(a, lds, lo) - (lo ? light_cdf(a, lds, lo - 1u) : 0.0);
    L = light_row(a, lds, lo);
    S = mk(0.0, 0.0, 0.0);
    centre = mk(0.0, 0.0, 0.0);
    u = 0.0;
    v = 0.0;
    if (L.kind <= LIGHT_TRIANGLE) {
        double ua = (double)xorwow_uniform(rng);
        double ub = (double)xorwow_uniform(rng);
        if (L.kind == LIGHT_TRIANGLE && ua + ub > 1.0) {
            ua = 1.0 - ua;
            ub = 1.0 - ub;
        }
        S = (load3(L.a) + ua * load3(L.b)) + ub * load3(L.c);
        const Vec D = S - P;
        const double d2 = dot(D, D);
        if (d2 > 0.0) {
            const double len = sqrt(d2);
            const Vec unit_d = over(D, len);
            const double c = fabs(dot(load3(L.n), unit_d));
            if (c != 0.0) {
                const double density = (d2 / (c * L.s)) * chance;
                if (usable_density(density)) {
                    valid = true;
                    dir = unit_d;
                    distance = len;
                    pdf = density;
                }
            }
        }
        u = ua;
        v = ub;
    } else {
        Vec p;
        double s;
        do {  // the lens loop of camera_ray
            const double da = (double)xorwow_uniform(rng);
            const double db = (double)xorwow_uniform(rng);
            p = mk(2.0 * da - 1.0, 2.0 * db - 1.0, 0.0);
            s = p.x * p.x + p.y * p.y;
        } while (!(s < 1.0 && s > 0.0));
        centre = light_centre(L, tm);
        const Vec oc = centre - P;
        const double d2 = dot(oc, oc), r2 = L.s * L.s;
        if (d2 > r2) {
            const Vec w = over(oc, sqrt(d2));
            const double cosmax = sqrt(1.0 - r2 / d2);
            const double omc = 1.0 - cosmax;
            const double z = 1.0 - s * omc;
            const double rho = sqrt(1.0 - z * z);
            const double q = sqrt(s);
            const double ex = (rho * p.x) / q, ey = (rho * p.y) / q;
            const double ax = fabs(w.x), ay = fabs(w.y), az = fabs(w.z);
            Vec e1;
            if (ax >= ay && ax >= az) e1 = over(mk(w.z, 0.0, -w.x), sqrt(w.z * w.z + w.x * w.x));
            else if (ay >= az) e1 = over(mk(-w.y, w.x, 0.0), sqrt(w.y * w.y + w.x * w.x));
            else e1 = over(mk(0.0, -w.z, w.y), sqrt(w.z * w.z + w.y * w.y));
            const Vec e2 = cross(w, e1);
            const Vec g = (z * w + ex * e1) + ey * e2;
            const Vec unit_d = over(g, sqrt(dot(g, g)));
            const Vec po = P - centre;
            const double qa = dot(unit_d, unit_d), qb = dot(po, unit_d), qc = dot(po, po) - r2;
            const double disc = qb * qb - qa * qc;
            const double len = (-qb - sqrt(disc)) / qa;
            const double density = chance / ((2.0 * kLightPi) * omc);
            if (omc != 0.0 && usable_density(density) && disc > 0.0 && len > 0.0) {
                valid = true;
                dir = unit_d;
                distance = len;
                pdf = density;
                S = P + len * unit_d;
            }
        }
    }
    return valid;
}

// what the lamp of a valid sample emits towards the point: its material's texture at S, at the sample's (u, v) or, for a sphere
// whose material reads them, at the sphere's own
template <class T>
DEV Vec light_emitted(const DeviceScene &sc, const LightRow &L, Vec S, Vec centre, double u, double v)
{
    const MatView mp = material_view<false>(sc, L.mat);
    if (L.kind >= LIGHT_SPHERE && mp.u32(MAT_OFF(needs_uv)) != 0) sphere_uv((1 / L.s) * (S - centre), u, v);
    return material_texture<T>(sc, mp, mp.u32(MAT_OFF(tex_inline)), u, v, S);
}

// the density with which a material of this kind sends a ray from a hit with shading normal n along the unit direction d, in
// closed form: 2 cos^3 / pi above a Lambertian surface, 1 / 4 pi for an isotropic medium; no other kind has one (0)
[[maybe_unused]] DEV double scatter_density(uint32_t kind, Vec n, Vec d)
{
    if (kind == MAT_LAMBERTIAN) {
        const double c = dot(n, d);
        return c > 0.0 ? (2.0 * ((c * c) * c)) / kLightPi : 0.0;
    }
    return kind == MAT_ISOTROPIC ? 1.0 / (4.0 * kLightPi) : 0.0;
}

// The environment's importance sampler (rt_scene_sample_environment, rt_scene_environment_pdf; the comment above env_sample_kernel
// says what the tables are): here because the three path kernels sample the environment too, where the scene makes it a light.
// STAGED: the caller holds the workgroup's copy of the first kEnvLdsRows entries
template <bool STAGED>
DEV double env_mcdf(const RT_CONST EnvRec *env, const double *lds, uint32_t j)
{
    if constexpr (STAGED) {
        if (j < kEnvLdsRows) return lds[j];
    }
    return env->mcdf[j];
}
// the density of the direction whose environment coordinates are e, (u, v); `texel`: j * width + i of its texel, -1 without tables
template <bool STAGED>
DEV double environment_density(const RT_CONST EnvRec *env, const double *lds, Vec e, double u, double v, int32_t &texel)
{
    texel = -1;
    if (!env->has_distribution) return 1.0 / (4.0 * kLightPi);
    int i, j;
    environment_texel(env->width, env->height, u, v, i, j);
    texel = j * env->width + i;
    const double pj = env_mcdf<STAGED>(env, lds, (uint32_t)j) - (j ? env_mcdf<STAGED>(env, lds, (uint32_t)j - 1u) : 0.0);
    const double *row = env->ccdf + (size_t)j * (size_t)env->width;
    const double pi = row[i] - (i ? row[i - 1] : 0.0);
    return ((pj * pi) * ((double)env->width * (double)env->height)) / (((2.0 * kLightPi) * kLightPi) * sqrt(1.0 - e.y * e.y));
}
// the first min(height, kEnvLdsRows) entries of the marginal table into the workgroup's copy; every lane, then one barrier
DEV void stage_environment(const RT_CONST EnvRec *env, double *mcdf_lds)
{
    if (env->has_distribution != 0) {
        const double *src = env->mcdf;
        const uint32_t n = min((uint32_t)env->height, kEnvLdsRows);
        for (uint32_t i = threadIdx.x; i < n; i += 256u) mcdf_lds[i] = src[i];
    }
    __syncthreads();
}
// The sample of rt_scene_sample_environment from its four draws (include/rtow.h states it operation by operation): with tables,
// xa bisects the marginal table for the row and xb that row's conditional table for the column, (xc, xd) place the direction
// inside the texel; without, (xc, xd) place it on the sphere uniformly.  Then R^T e, and the density -- and, where asked for, the
// value -- from that final direction through the environment's own lookup (environment_coords): the sample's pdf is
// environment_pdf of its direction, and what a path along it adds at its miss.  `texel` is the one the bisections named.  Returns
// validity; an invalid sample leaves dir (0, 0, 0), pdf 0 and emitted (0, 0, 0).  Termination: each bisection halves hi - lo.
template <class T>
DEV bool environment_sample(const DeviceScene &sc, const RT_CONST EnvRec *env, const double *mcdf_lds, double xa, double xb, double xc, double xd,
                            bool want_emitted, Vec &dir, double &pdf, Vec &emitted, int32_t &texel)
{
    const uint32_t width = (uint32_t)env->width, height = (uint32_t)env->height;
    Vec e;
    texel = -1;
    if (env->has_distribution != 0) {
        uint32_t lo = 0, hi = height - 1u;
        while (lo < hi) {  // the first row with mcdf >= xa (the last entry is 1.0 >= xa)
            const uint32_t mid = (lo + hi) / 2u;
            if (env_mcdf<true>(env, mcdf_lds, mid) >= xa) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t j = lo;
        const double *row = env->ccdf + (size_t)j * width;
        lo = 0;
        hi = width - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2u;
            if (row[mid] >= xb) hi = mid;
            else lo = mid + 1u;
        }
        const uint32_t i = lo;
        texel = (int32_t)(j * width + i);
        const double u = ((double)i + xc) / (double)width;
        const double v = 1.0 - ((double)j + xd) / (double)height;
        const double theta = kLightPi * v, phi = (2.0 * kLightPi) * u - kLightPi;
        const double st = sin(theta);
        e = mk(st * cos(phi), -cos(theta), -(st * sin(phi)));
    } else {  // no tables: the sphere uniformly
        const double y = 1.0 - 2.0 * xc;
        const double st = sqrt(1.0 - y * y), phi = (2.0 * kLightPi) * xd - kLightPi;
        e = mk(st * cos(phi), y, -(st * sin(phi)));
    }
    // R^T e, each row (a + b) + c
    dir = mk((env->rot[0] * e.x + env->rot[3] * e.y) + env->rot[6] * e.z, (env->rot[1] * e.x + env->rot[4] * e.y) + env->rot[7] * e.z,
             (env->rot[2] * e.x + env->rot[5] * e.y) + env->rot[8] * e.z);
    // density and value from the direction itself, through the environment's own lookup
    Vec el;
    double u, v;
    environment_coords(env, dir, el, u, v);
    int32_t seen;
    pdf = environment_density<true>(env, mcdf_lds, el, u, v, seen);
    const bool valid = usable_density(pdf);
    emitted = mk(0.0, 0.0, 0.0);
    if (!valid) {
        dir = mk(0.0, 0.0, 0.0);
        pdf = 0.0;
    }
    if (valid && want_emitted) emitted = environment_lookup<T>(sc, env, el, u, v);
    return valid;
}

// What a path that scattered from a Lambertian or isotropic hit (kind, normal) into `ray` does about the lights (include/rtow.h
// rt_scene_path_advance_direct; the three path kernels): the three functions above for the point ray.o at the time ray.tm, drawn
// from the path's stream; contribution = (scatter / pdf) * emitted.  Returns sampled, contribution != 0: then the sample waits to be
// weighted behind the density loop, which is asked along it (along_o, along_d, along_tm), with light = next * contribution (next:
// the path's throughput behind this bounce), other = its scatter density and `distance` where a shadow ray along it meets the lamp.
// sent_next: the density with which the material sent the scattered ray where it goes, the closed form for its unit direction.
// SHARED (a scene whose environment is a light too): the table gets the share `share` = c_l of the samples, contribution =
// (scatter / (share * pdf)) * emitted.
template <class T, bool SHARED = false>
DEV bool path_light_sample(const DeviceScene &sc, const LightArgs &la, const LightLds &lds, const Ray &ray, uint32_t kind, Vec normal, Vec next,
                           Xorwow &rng, Vec &along_o, Vec &along_d, double &along_tm, Vec &light, double &other, double &distance, double &sent_next,
                           double share = 1.0)
{
    const Vec P = ray.o;
    const double tm = ray.tm;
    uint32_t row;
    LightRow L;
    Vec dir, S, centre, contribution = mk(0.0, 0.0, 0.0);
    double pdf, u, v, scatter = 0.0;
    if (light_sample(la, lds, P, tm, rng, row, L, dir, distance, pdf, S, centre, u, v)) {
        const Vec emitted = light_emitted<T>(sc, L, S, centre, u, v);
        scatter = scatter_density(kind, normal, dir);
        if constexpr (SHARED) {
            if (scatter != 0.0) contribution = (scatter / (share * pdf)) * emitted;
        } else {
            if (scatter != 0.0) contribution = (scatter / pdf) * emitted;
        }
    }
    const bool sampled = contribution.x != 0.0 || contribution.y != 0.0 || contribution.z != 0.0;
    if (sampled) {
        along_o = P;
        along_d = dir;
        along_tm = tm;
        light = next * contribution;
        other = scatter;
    }
    const Vec unit_next = (1 / sqrt((ray.d.x * ray.d.x + ray.d.y * ray.d.y) + ray.d.z * ray.d.z)) * ray.d;
    sent_next = scatter_density(kind, normal, unit_next);
    return sampled;
}

// The same where the pick fell on the environment (SCENE_ENVIRONMENT_LIGHT; include/rtow.h rt_scene_path_advance_direct): the sample
// of rt_scene_sample_environment, four draws from the path's stream; contribution = (scatter / (share * pdf)) * emitted with share =
// c_e.  The out-parameters are path_light_sample's, distance = +inf (the shadow ray runs to the end of the world), and `own` = share *
// pdf: the density the sample is weighted with, which is this lane's alone -- no loop over the light table runs for it.
template <class T>
DEV bool path_environment_sample(const DeviceScene &sc, const RT_CONST EnvRec *env, const double *mcdf_lds, const Ray &ray, uint32_t kind, Vec normal,
                                 Vec next, Xorwow &rng, Vec &along_o, Vec &along_d, double &along_tm, Vec &light, double &other, double &distance,
                                 double &sent_next, double share, double &own)
{
    const double xa = (double)xorwow_uniform(rng);
    const double xb = (double)xorwow_uniform(rng);
    const double xc = (double)xorwow_uniform(rng);
    const double xd = (double)xorwow_uniform(rng);
    Vec dir, emitted, contribution = mk(0.0, 0.0, 0.0);
    double pdf, scatter = 0.0;
    int32_t texel;
    if (environment_sample<T>(sc, env, mcdf_lds, xa, xb, xc, xd, true, dir, pdf, emitted, texel)) {
        scatter = scatter_density(kind, normal, dir);
        if (scatter != 0.0) contribution = (scatter / (share * pdf)) * emitted;
    }
    const bool sampled = contribution.x != 0.0 || contribution.y != 0.0 || contribution.z != 0.0;
    if (sampled) {
        along_o = ray.o;
        along_d = dir;
        along_tm = ray.tm;
        light = next * contribution;
        other = scatter;
        distance = (double)INFINITY;
        own = share * pdf;
    }
    const Vec unit_next = (1 / sqrt((ray.d.x * ray.d.x + ray.d.y * ray.d.y) + ray.d.z * ray.d.z)) * ray.d;
    sent_next = scatter_density(kind, normal, unit_next);
    return sampled;
}
// What the two ends of a path and the sample site of the three kernels share under SCENE_ENVIRONMENT_LIGHT.
// the density with which an environment sample would have drawn the incoming direction of a path that ends in a miss: c_e *
// rt_scene_environment_pdf's value, through environment_coords again (bounce() keeps its signature, the plain lane units their text)
[[maybe_unused]] DEV double environment_end_density(const RT_CONST EnvRec *env, const double *mcdf_lds, Vec d)
{
    Vec e;
    double u, v;
    environment_coords(env, d, e, u, v);
    int32_t texel;
    const double pdf = environment_density<true>(env, mcdf_lds, e, u, v, texel);
    return env->light_share * (usable_density(pdf) ? pdf : 0.0);
}
// The workgroup's copy of the marginal table for a path kernel compiled for such scenes (ENV), staged as env_sample_kernel stages
// it: 16 KB beside the light rows.  Every lane comes here; the barrier is stage_environment's.  nullptr in the other instantiations,
// which hold no such array.
template <bool ENV>
DEV const double *staged_environment(const DeviceScene &sc)
{
    if constexpr (ENV) {
        __shared__ double mcdf_lds[kEnvLdsRows];
        stage_environment(environment_of(sc.camera), mcdf_lds);
        return mcdf_lds;
    } else {
        return nullptr;
    }
}
// The sample site: the pick (one draw where the table has a share, none where c_e == 1), then one of the two samplers.  `table`:
// the sample waits for the table's density (mixture_density); otherwise `own` holds its density.
template <class T>
DEV bool path_emitter_sample(const DeviceScene &sc, const LightArgs &la, const LightLds &lds, const RT_CONST EnvRec *env, const double *mcdf_lds,
                             const Ray &ray, uint32_t kind, Vec normal, Vec next, Xorwow &rng, Vec &along_o, Vec &along_d, double &along_tm,
                             Vec &light, double &other, double &distance, double &sent_next, bool &table, double &own)
{
    const double c_e = env->light_share;
    bool sky = true;
    if (c_e < 1.0 && la.n_lights != 0) {  // (c_e < 1 only where the table has rows: scene_builder.cpp build_environment)
        const double x = (double)xorwow_uniform(rng);
        sky = x <= c_e;
    }
    table = false;
    if (sky) return path_environment_sample<T>(sc, env, mcdf_lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other, distance, sent_next, c_e, own);
    table = path_light_sample<T, true>(sc, la, lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other, distance, sent_next, env->table_share);
    return table;
}

// The mixture density of rt_scene_light_pdf along the ray (o, d) at the time tm: the sum over the table of each light's chance
// times the density with which light_sample would have drawn the direction d from o, where the ray meets the light (a plane
// inside the parallelogram or triangle, a sphere seen from outside in front of o).  Wave-uniform: every lane on row i, an LDS
// broadcast below the cap.  NEAREST (light_pdf_kernel): also the row of the usable light met at the smallest parameter, or -1,
// into *nearest_light -- a template argument because the compiler did not drop the sphere's root and the comparison from the
// path kernels, which ask for neither, when it was a null pointer (81 instructions in advance_direct's strict unit).  The loop
// runs n_lights times.
template <bool NEAREST = false>
DEV double mixture_density(const LightArgs &a, const LightLds &lds, Vec o, Vec d, double tm, int32_t *nearest_light = nullptr)
{
    const double dd = dot(d, d);
    double sum = 0.0, nearest = (double)INFINITY, before = 0.0;
    int32_t light = -1;
    for (uint32_t i = 0; i < a.n_lights; i++) {
        const LightRow L = light_row(a, lds, i);
        const double upto = light_cdf(a, lds, i);
        const double chance = upto - before;
        before = upto;
        double density = 0.0, t = 0.0;
        if (L.kind <= LIGHT_TRIANGLE) {
            const Vec n = load3(L.n), Q = load3(L.a), U = load3(L.b), V = load3(L.c);
            const double denom = dot(n, d);
            if (denom != 0.0) {
                t = dot(n, Q - o) / denom;
                if (t > 0.0) {
                    const Vec ph = (o + t * d) - Q;
                    const Vec m = cross(U, V);
                    const double mm = dot(m, m);
                    const double alpha = dot(m, cross(ph, V)) / mm, beta = dot(m, cross(U, ph)) / mm;
                    const bool below = L.kind == LIGHT_TRIANGLE ? alpha + beta <= 1.0 : (alpha <= 1.0 && beta <= 1.0);
                    if (0.0 <= alpha && 0.0 <= beta && below) density = (((t * t) * dd) / ((fabs(denom) / sqrt(dd)) * L.s)) * chance;
                }
            }
        } else {
            const Vec oc = light_centre(L, tm) - o;
            const double d2 = dot(oc, oc), r2 = L.s * L.s;
            if (d2 > r2) {
                const double b = dot(oc, d);
                const double disc = b * b - dd * (d2 - r2);
                if (b > 0.0 && disc >= 0.0) {
                    const double omc = 1.0 - sqrt(1.0 - r2 / d2);
                    if (omc != 0.0) density = chance / ((2.0 * kLightPi) * omc);
                    if constexpr (NEAREST) t = (b - sqrt(disc)) / dd;
                }
            }
        }
        if (usable_density(density)) {
            sum = sum + density;
            if constexpr (NEAREST) {
                if (t < nearest) {
                    nearest = t;
                    light = (int32_t)i;
                }
            }
        }
    }
    if constexpr (NEAREST) *nearest_light = light;
    return sum;
}
}  // namespace
#endif

#if RT_LIGHTS
template <int STRICT, class T>
__global__ __launch_bounds__(256) void light_sample_kernel(DeviceScene sc, LightArgs a)
{
    __shared__ __attribute__((aligned(16))) double rows_lds[kLightLdsRows * kLightRowDoubles];
    __shared__ __attribute__((aligned(16))) double cdf_lds[kLightLdsRows];
    __shared__ uint32_t wave_valid[4];
    global_tables_only(sc);
    stage_lights(a, rows_lds, cdf_lds);
    const LightLds lds{rows_lds, cdf_lds};
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (k < a.count) {
        // the point and the six words are read here, before anything is written: rng_out may be rng_in
        const Vec P = load3(a.point + (size_t)k * 3);
        const double tm = a.time ? a.time[k] : a.time_all;
        Xorwow rng = lane_stream(a, k);
        Vec dir = mk(0.0, 0.0, 0.0), emitted = mk(0.0, 0.0, 0.0), contribution = mk(0.0, 0.0, 0.0);
        double distance = 0.0, pdf = 0.0, scatter = 0.0;
        int32_t light = -1;
        if (a.n_lights != 0) {
            uint32_t row;
            LightRow L;
            Vec S, centre;
            double u, v;
            valid = light_sample(a, lds, P, tm, rng, row, L, dir, distance, pdf, S, centre, u, v);
            light = (int32_t)row;
            if (valid && (a.emitted || a.contribution)) emitted = light_emitted<T>(sc, L, S, centre, u, v);
            if (valid && (a.scatter_pdf || a.contribution)) {
                const uint32_t kind = a.material[k];
                scatter = scatter_density(kind, kind == MAT_LAMBERTIAN ? load3(a.normal + (size_t)k * 3) : mk(0.0, 0.0, 0.0), dir);  // (only it reads the normal)
                if (scatter != 0.0) contribution = (scatter / pdf) * emitted;
            }
        }
        if (a.direction) store3(a.direction, k, dir);
        if (a.distance) a.distance[k] = distance;
        if (a.light) a.light[k] = light;
        if (a.pdf) a.pdf[k] = pdf;
        if (a.emitted) store3(a.emitted, k, emitted);
        if (a.scatter_pdf) a.scatter_pdf[k] = scatter;
        if (a.contribution) store3(a.contribution, k, contribution);
        if (a.rng_out) store_stream(a.rng_out + (size_t)k * 6, 1, rng);
    }
    count_valid(a.valid_counter, valid, wave_valid);
}

template <int STRICT>
__global__ __launch_bounds__(256) void light_pdf_kernel(DeviceScene sc, LightArgs a)
{
    __shared__ __attribute__((aligned(16))) double rows_lds[kLightLdsRows * kLightRowDoubles];
    __shared__ __attribute__((aligned(16))) double cdf_lds[kLightLdsRows];
    __shared__ uint32_t wave_valid[4];
    stage_lights(a, rows_lds, cdf_lds);
    const LightLds lds{rows_lds, cdf_lds};
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = k < a.count;
    const size_t at3 = mine ? (size_t)k * 3 : 0;  // (a lane beyond the count reads ray 0 and writes nothing: the loop stays wave-uniform)
    const Vec o = load3(a.point + at3), d = load3(a.direction_in + at3);
    const double tm = a.time ? a.time[mine ? k : 0] : a.time_all;
    int32_t light;
    const double sum = mixture_density<true>(a, lds, o, d, tm, &light);
    if (mine) {
        if (a.pdf) a.pdf[k] = sum;
        if (a.light) a.light[k] = light;
    }
    count_valid(a.valid_counter, mine && light >= 0, wave_valid);
}

// ------------------------------------------------------------------------------------------------
// Environment sampling (rt_scene_sample_environment, rt_scene_environment_pdf; include/rtow.h states both operation by operation,
// tests/environment_restated.py restates the strict build).  One lane a point or a ray, the light calls' arrays (LightArgs: no
// light table, no strategy).  The tables are the EnvRec's: a marginal table over the rows of the map and one conditional table a
// row.  A sample bisects both, log2 H + log2 W dependent loads a lane: a workgroup first stages the first kEnvLdsRows entries of
// the marginal table in LDS with coalesced loads (flat_scene.h says why that many), so the first chain is LDS reads; the chain
// through the lane's own conditional row stays in global memory -- 64 lanes stand on up to 64 rows of W doubles, which no LDS
// holds.  Rows of the marginal table beyond the cap are read from global memory.  The density is one expression, of the texel the
// environment's own lookup names for the direction: the sample's pdf is environment_pdf of its direction.  No lane returns early
// (all meet at the barriers); the count of valid results reduces as the light kernels' does.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T>
__global__ __launch_bounds__(256) void env_sample_kernel(DeviceScene sc, LightArgs a)
{
    __shared__ double mcdf_lds[kEnvLdsRows];
    __shared__ uint32_t wave_valid[4];
    global_tables_only(sc);
    const RT_CONST EnvRec *env = environment_of(sc.camera);
    stage_environment(env, mcdf_lds);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (k < a.count) {
        // the six words are read here, before anything is written: rng_out may be rng_in
        Xorwow rng = lane_stream(a, k);
        const double xa = (double)xorwow_uniform(rng);
        const double xb = (double)xorwow_uniform(rng);
        const double xc = (double)xorwow_uniform(rng);
        const double xd = (double)xorwow_uniform(rng);
        Vec dir, emitted, contribution = mk(0.0, 0.0, 0.0);
        double pdf, scatter = 0.0;
        int32_t texel;
        valid = environment_sample<T>(sc, env, mcdf_lds, xa, xb, xc, xd, a.emitted || a.contribution, dir, pdf, emitted, texel);
        if (valid && (a.scatter_pdf || a.contribution)) {
            const uint32_t kind = a.material[k];
            scatter = scatter_density(kind, kind == MAT_LAMBERTIAN ? load3(a.normal + (size_t)k * 3) : mk(0.0, 0.0, 0.0), dir);  // (only it reads the normal)
            if (scatter != 0.0) contribution = (scatter / pdf) * emitted;
        }
        if (a.direction) store3(a.direction, k, dir);
        if (a.distance) a.distance[k] = valid ? (double)INFINITY : 0.0;
        if (a.light) a.light[k] = texel;
        if (a.pdf) a.pdf[k] = pdf;
        if (a.emitted) store3(a.emitted, k, emitted);
        if (a.scatter_pdf) a.scatter_pdf[k] = scatter;
        if (a.contribution) store3(a.contribution, k, contribution);
        if (a.rng_out) store_stream(a.rng_out + (size_t)k * 6, 1, rng);
    }
    count_valid(a.valid_counter, valid, wave_valid);
}

template <int STRICT>
__global__ __launch_bounds__(256) void env_pdf_kernel(DeviceScene sc, LightArgs a)
{
    __shared__ uint32_t wave_valid[4];
    const RT_CONST EnvRec *env = environment_of(sc.camera);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (k < a.count) {
        Vec e;
        double u, v;
        environment_coords(env, load3(a.direction_in + (size_t)k * 3), e, u, v);
        int32_t texel;
        double pdf = environment_density<false>(env, nullptr, e, u, v, texel);
        valid = usable_density(pdf);
        if (!valid) pdf = 0.0;
        if (a.pdf) a.pdf[k] = pdf;
        if (a.light) a.light[k] = texel;
    }
    count_valid(a.valid_counter, valid, wave_valid);
}

hipError_t RT_CAT(launch_env_sample_, RT_SUFFIX)(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    const bool any = a.direction || a.distance || a.light || a.pdf || a.emitted || a.scatter_pdf || a.contribution || a.rng_out;
    if (!info && (!any || !(sc.flags & SCENE_ENVIRONMENT))) return hipErrorInvalidValue;
    if (!info && (a.scatter_pdf || a.contribution) && (!a.normal || !a.material)) return hipErrorInvalidValue;
    return info_or_launch(env_sample_kernel<RT_STRICT, TListNested>, sc, a, a.count, stream, info);
}
hipError_t RT_CAT(launch_env_pdf_, RT_SUFFIX)(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    if (!info && (!a.direction_in || !(a.pdf || a.light) || !(sc.flags & SCENE_ENVIRONMENT))) return hipErrorInvalidValue;
    return info_or_launch(env_pdf_kernel<RT_STRICT>, sc, a, a.count, stream, info);
}

hipError_t RT_CAT(launch_light_sample_, RT_SUFFIX)(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    const bool any = a.direction || a.distance || a.light || a.pdf || a.emitted || a.scatter_pdf || a.contribution || a.rng_out;
    if (!info && (!a.point || !any || !a.rows || !a.cdf)) return hipErrorInvalidValue;
    if (!info && (a.scatter_pdf || a.contribution) && (!a.normal || !a.material)) return hipErrorInvalidValue;
    return info_or_launch(light_sample_kernel<RT_STRICT, TListNested>, sc, a, a.count, stream, info);
}
hipError_t RT_CAT(launch_light_pdf_, RT_SUFFIX)(const DeviceScene &sc, const LightArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    if (!info && (!a.point || !a.direction_in || !(a.pdf || a.light) || !a.rows || !a.cdf)) return hipErrorInvalidValue;
    return info_or_launch(light_pdf_kernel<RT_STRICT>, sc, a, a.count, stream, info);
}
#elif RT_ADVANCE_DIRECT
// ------------------------------------------------------------------------------------------------
// Path advances with light samples (rt_scene_path_advance_direct; include/rtow.h states the operation), launches 1 and 2 of 4
// (render_iface.h AdvanceDirectArgs).  The world is searched twice for a row that scatters from a diffuse hit -- once for the
// path, once for the shadow ray -- and the two searches are two kernels: one kernel with both would hold the registers and the
// scratch of the larger through the other, and every lane whose path ended would idle through the second.
//   advance_direct_kernel: advance_kernel's iteration (its search in text, bounce); then, for a row that scattered from a Lambertian or
//   isotropic hit, path_light_sample from the path's own stream; then, every lane of the wave here again, mixture_density for the
//   one density a lane can need: along its incoming ray where it ended on a lamp with a density carried in, along its sample
//   where it scattered.  A wave in which no lane needs one skips the loop.  The table is staged in LDS as the light kernels stage it.
//   shadow_kernel: query_kernel's occlusion search (query_search) for the rows launch 1 left pending.
// ENV (the launcher's choice for a scene with SCENE_ENVIRONMENT_LIGHT; every other scene runs the instantiations without it, whose
// code holds none of this): the environment is a light too.  The sample site picks between it and the table (path_emitter_sample),
// a miss with a density carried in is a second kind of weighted end, whose density is the lane's own, and only the lanes that
// need the TABLE's density -- a lamp end, a table sample -- vote for the loop; the marginal table's first kEnvLdsRows entries are
// staged beside the light rows (staged_environment: every lane, one barrier, none behind it).
// No lane returns before a barrier, no workgroup waits for another.  Termination: as for advance_kernel, and as light_sample,
// mixture_density and query_search say; the two bisections of an environment sample each halve hi - lo.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T, bool ENV = false>
__global__ __launch_bounds__(256) void advance_direct_kernel(DeviceScene sc, AdvanceDirectArgs d)
{
    __shared__ __attribute__((aligned(16))) double rows_lds[kLightLdsRows * kLightRowDoubles];
    __shared__ __attribute__((aligned(16))) double cdf_lds[kLightLdsRows];
    __shared__ uint32_t wave_survivors[4];
    global_tables_only(sc);
    const AdvanceArgs &a = d.adv;
    LightArgs la{};  // what the table's readers take
    la.rows = d.rows;
    la.cdf = d.cdf;
    la.n_lights = d.n_lights;
    stage_lights(la, rows_lds, cdf_lds);
    const LightLds lds{rows_lds, cdf_lds};
    [[maybe_unused]] const double *mcdf_lds = staged_environment<ENV>(sc);
    [[maybe_unused]] const RT_CONST EnvRec *env = environment_of(sc.camera);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = a.count_in ? min(*a.count_in, a.capacity) : a.capacity;
    const bool stepped = k < n && (!a.alive || a.alive[k] != 0);
    bool scattered = false, lamp = false, sampled = false;
    [[maybe_unused]] bool sky = false, table = false;  // ENV: a miss weighted like a lamp end; the sample waits for the table's density
    [[maybe_unused]] double own = 0.0;                 // ENV: the density of a sky end or of an environment sample, this lane's alone
    // what the density loop and the fold behind it read: the ray the density is asked along, the row's id, its light and weights
    Vec along_o = mk(0.0, 0.0, 0.0), along_d = mk(0.0, 0.0, 1.0), light = mk(0.0, 0.0, 0.0);
    double along_tm = 0.0, other = 0.0, distance = 0.0;
    int32_t id = -1;
    if (stepped) {
        Ray ray = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
        Xorwow rng = lane_stream(a, k);
        const NodeView nv{sc.nodes, 0u, false};
        Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
        HitInfo h;
        h.t = 0.0;
        h.ref = kNone;
        h.obj = kNone;
        bool hit = false;
        if constexpr (T::WORLD == 0) {
            if (sc.n_world_nodes != 0) {
                Walk w{};
                walk_begin<false>(w, ray, DBL_MAX);
                while (w.state != kNone) {
                    if (walk_moving(w.state)) walk_node<false>(nv, ray, 0.001, w);
                    else walk_leaves<T>(sc, nv, ray, 0.001, w, h, rng);
                }
                hit = w.any;
            }
        } else {
            hit = world_hit_list<T>(sc, ray, 0.001, DBL_MAX, h, rng);
        }
        Vec normal;
        uint32_t kind;
        bool front;
        scattered = bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, true, true, normal, front, kind);
        const Vec carried = a.throughput ? mk(a.throughput[(size_t)k * 3 + 0], a.throughput[(size_t)k * 3 + 1], a.throughput[(size_t)k * 3 + 2])
                                         : mk(1.0, 1.0, 1.0);
        id = a.ray_id ? a.ray_id[k] : (int32_t)k;
        const double sent = d.scatter_pdf ? d.scatter_pdf[k] : 0.0;  // the density the bounce before sent this ray with
        if (!scattered) {
            lamp = hit && kind == MAT_DIFFUSE_LIGHT && sent > 0.0 && a.radiance && id >= 0 && (uint32_t)id < a.sources;
            if constexpr (ENV) sky = !hit && sent > 0.0 && a.radiance && id >= 0 && (uint32_t)id < a.sources;
            if (lamp) {  // weighted behind the density loop, along the incoming ray as given
                along_o = ray.o;
                along_d = ray.d;
                along_tm = ray.tm;
                light = carried * accumulated;
                other = sent;
            } else if (sky) {  // weighted against the environment sample the bounce before could have taken: no loop
                own = environment_end_density(env, mcdf_lds, ray.d);
                light = carried * accumulated;
                other = sent;
            } else if (a.radiance && id >= 0 && (uint32_t)id < a.sources) {  // w = 1: the plain advance's fold
                const Vec product = carried * accumulated;
                double *row = a.radiance + (size_t)id * 3;
                const Vec sum = mk(row[0], row[1], row[2]) + product;
                row[0] = sum.x;
                row[1] = sum.y;
                row[2] = sum.z;
            }
        } else {
            const Vec next = carried * throughput;
            double sent_next = 0.0;
            if constexpr (ENV) {
                if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && d.sample != 0) {
                    sampled = path_emitter_sample<T>(sc, la, lds, env, mcdf_lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other,
                                                     distance, sent_next, table, own);
                }
            } else if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && d.n_lights != 0 && d.sample != 0) {
                sampled = path_light_sample<T>(sc, la, lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other, distance, sent_next);
            }
            if (a.stage.origin) store3(a.stage.origin, k, ray.o);
            if (a.stage.direction) store3(a.stage.direction, k, ray.d);
            if (a.stage.time) a.stage.time[k] = ray.tm;
            if (a.stage.rng_state) store_stream(a.stage.rng_state + (size_t)k * 6, 1, rng);  // the stream after the last draw, the sample's included
            if (a.stage.throughput) store3(a.stage.throughput, k, next);
            if (a.stage.ray_id) a.stage.ray_id[k] = id;
            if (a.stage.t) a.stage.t[k] = h.t;
            if (a.stage.normal) store3(a.stage.normal, k, normal);
            if (a.stage.front_face) a.stage.front_face[k] = front ? 1 : 0;
            if (a.stage.material) a.stage.material[k] = (uint8_t)kind;
            d.scatter_pdf_stage[k] = sent_next;
        }
    }
    // every lane of the workgroup is here again.  The mixture density along `along`, every lane of the wave on the same row (a lane
    // that needs none runs the loop on a ray of its own that meets what it meets: its sum is not read)
    double density_sum = 0.0;
    if constexpr (ENV) {  // only the lanes that need the TABLE's density vote: a wave whose lanes all picked the sky skips the loop, and so does
        // every wave where the table has no share (chance 1 beside lamps: c_l * sum is 0 without walking the table, a lamp end's w = q / q)
        if (env->table_share != 0.0 && __ballot(lamp || table) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
        density_sum = lamp || table ? env->table_share * density_sum : own;  // p of include/rtow.h, per emitter
        lamp = lamp || sky;
    } else {
        if (__ballot(lamp || sampled) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
    }
    if (lamp) {  // w = q / (q + p): the scattered ray found the lamp a light sample of the bounce before could have found
        const double w = other / (other + density_sum);
        double *row = a.radiance + (size_t)id * 3;
        const Vec sum = mk(row[0], row[1], row[2]) + w * light;
        row[0] = sum.x;
        row[1] = sum.y;
        row[2] = sum.z;
    }
    if (sampled) {  // w = p / (p + s); the shadow ray decides in launch 2
        const double both = density_sum + other;
        const double w = both == 0.0 ? 0.0 : density_sum / both;
        store3(d.shadow_direction, k, along_d);
        d.shadow_distance[k] = distance;
        store3(d.shadow_radiance, k, w * light);
    }
    if (k < a.capacity) d.pending[k] = sampled ? 1 : 0;
    if (d.shadow_counters) {  // one atomic per wave
        const unsigned long long cast = __ballot(sampled);
        if ((threadIdx.x & 63u) == 0 && cast) atomicAdd(d.shadow_counters, (unsigned long long)__popcll(cast));
    }
    count_survivors(a, k, stepped, scattered, wave_survivors);
}

// Launch 2: row k's shadow ray (staged origin, shadow direction, staged time) over (0.001, distance * (1 - 2^-20)), searched as
// query_kernel searches in occlusion mode.  Only a medium's test draws: from the row's staged stream, which is written back.
template <int STRICT, class T>
__global__ __launch_bounds__(256) void shadow_kernel(DeviceScene sc, AdvanceDirectArgs d)
{
    global_tables_only(sc);
    const AdvanceArgs &a = d.adv;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool pending = k < a.capacity && d.pending[k] != 0;
    if (__ballot(pending) == 0ull) return;  // (the whole wave: no barrier in this kernel)
    bool reached = false;
    if (pending) {
        Ray ray;
        ray.o = mk(a.stage.origin[(size_t)k * 3 + 0], a.stage.origin[(size_t)k * 3 + 1], a.stage.origin[(size_t)k * 3 + 2]);
        ray.d = mk(d.shadow_direction[(size_t)k * 3 + 0], d.shadow_direction[(size_t)k * 3 + 1], d.shadow_direction[(size_t)k * 3 + 2]);
        ray.tm = a.stage.time[k];
        const double tmax = fmin(d.shadow_distance[k] * (1.0 - 0x1p-20), DBL_MAX);
        const bool media = (sc.flags & SCENE_HAS_MEDIA) != 0;
        Xorwow rng{};
        uint32_t *w = a.stage.rng_state + (size_t)k * 6;
        if (media) rng = load_stream(w, 1);
        HitInfo h;
        uint32_t leaf = kNone;
        reached = !query_search<T>(sc, d.node_leaf_pos, ray, 0.001, tmax, !media, h, leaf, rng);  // a medium's answer depends on what was found before it: the full search
        if (media) store_stream(w, 1, rng);
        const int32_t id = a.stage.ray_id[k];
        if (reached && a.radiance && id >= 0 && (uint32_t)id < a.sources) {
            double *row = a.radiance + (size_t)id * 3;
            const Vec sum = mk(row[0], row[1], row[2]) +
                            mk(d.shadow_radiance[(size_t)k * 3 + 0], d.shadow_radiance[(size_t)k * 3 + 1], d.shadow_radiance[(size_t)k * 3 + 2]);
            row[0] = sum.x;
            row[1] = sum.y;
            row[2] = sum.z;
        }
    }
    if (d.shadow_counters) {  // one atomic per wave
        const unsigned long long found = __ballot(reached);
        if ((threadIdx.x & 63u) == 0 && found) atomicAdd(d.shadow_counters + 1, (unsigned long long)__popcll(found));
    }
}

hipError_t RT_CAT(launch_advance_direct_, RT_SUFFIX)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_advance_direct_, sc, a, stream, info);
    const AdvanceArgs &v = a.adv;
    if (!info && (!v.origin || !v.direction || !v.survivor || !v.block_counts || !v.stage.origin || !v.stage.time || !v.stage.rng_state ||
                  !v.stage.ray_id || !a.scatter_pdf_stage || !a.shadow_direction || !a.shadow_distance || !a.shadow_radiance || !a.pending))
        return hipErrorInvalidValue;
    if (!info && a.n_lights != 0 && (!a.rows || !a.cdf)) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, AdvanceDirectArgs) =
        sc.world_kind == WORLD_BVH ? advance_direct_kernel<RT_STRICT, TBvhNested> : advance_direct_kernel<RT_STRICT, TListNested>;
    if (sc.flags & SCENE_ENVIRONMENT_LIGHT)  // the instantiations that sample the environment too; every other scene launches what it did
        kernel = sc.world_kind == WORLD_BVH ? advance_direct_kernel<RT_STRICT, TBvhNested, true> : advance_direct_kernel<RT_STRICT, TListNested, true>;
    return info_or_launch(kernel, sc, a, v.capacity, stream, info);
}

hipError_t RT_CAT(launch_advance_shadow_, RT_SUFFIX)(const DeviceScene &sc, const AdvanceDirectArgs &a, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_advance_shadow_, sc, a, stream, info);
    const AdvanceArgs &v = a.adv;
    if (!info && (!v.stage.origin || !v.stage.time || !v.stage.rng_state || !v.stage.ray_id || !a.shadow_direction || !a.shadow_distance ||
                  !a.shadow_radiance || !a.pending))
        return hipErrorInvalidValue;
    if (!info && sc.world_kind == WORLD_BVH && !a.node_leaf_pos) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, AdvanceDirectArgs) =
        sc.world_kind == WORLD_BVH ? shadow_kernel<RT_STRICT, TBvhNested> : shadow_kernel<RT_STRICT, TListNested>;
    return info_or_launch(kernel, sc, a, v.capacity, stream, info);
}
#elif RT_RADIANCE_DIRECT
// ------------------------------------------------------------------------------------------------
// Radiance queries with light samples (rt_scene_radiance_direct; include/rtow.h states the operation): the estimator of max_depth
// calls of rt_scene_path_advance_direct, folded over `samples` paths a ray, in radiance_kernel's one flattened loop -- one launch,
// no workspace, no compaction.  An iteration is ONE world search for every lane still in the loop: of its path ray over
// (0.001, DBL_MAX), or of the shadow ray its last bounce left pending over (0.001, distance * (1 - 2^-20)), both through
// query_search, which takes the interval and the early exit as arguments -- lanes in the two phases share the search code, and no
// lane idles through a second search.  The state beside the search is one path's: the shadow ray shares the path ray's origin and
// time, so a pending sample costs its direction, its end and its weighted light (seven doubles).
//   after a path search: advance_direct_kernel's step, light sample and fold -- bounce from throughput (1, 1, 1) and accumulated
//   (0, 0, 0), the carried throughput multiplied in behind it, as the advance does, then path_light_sample;
//   then, every lane still in the loop here again, mixture_density over the LDS-staged light table, every lane on the same row,
//   skipped where no lane of the wave needs a density (a lane in its shadow phase never does);
//   after a shadow search: the parked light is added where nothing was found, and the lane is back on its path ray.
// A path ends only where no sample is pending (an ended path draws none, the last bounce takes none): it folds into the sum and the
// next sample starts in the same iteration.  Every lane, k >= count included, reaches the barriers of stage_lights; there is none
// behind them.  ENV: as advance_direct_kernel says -- the pick at the sample site, the weighted miss, the ballot of the lanes that
// need the table's density, the marginal table staged behind the light rows' barrier by every lane.  Termination: at most
// samples * max_depth path searches and as many shadow searches, each bounded (the argument on the two searches), each followed by
// bounded helpers; the two bisections of an environment sample each halve hi - lo.
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T, bool ENV = false>
__global__ __launch_bounds__(256) void radiance_direct_kernel(DeviceScene sc, RadianceDirectArgs d)
{
    __shared__ __attribute__((aligned(16))) double rows_lds[kLightLdsRows * kLightRowDoubles];
    __shared__ __attribute__((aligned(16))) double cdf_lds[kLightLdsRows];
    global_tables_only(sc);
    const RadianceArgs &a = d.rad;
    LightArgs la{};  // what the table's readers take
    la.rows = d.rows;
    la.cdf = d.cdf;
    la.n_lights = d.n_lights;
    stage_lights(la, rows_lds, cdf_lds);
    const LightLds lds{rows_lds, cdf_lds};
    [[maybe_unused]] const double *mcdf_lds = staged_environment<ENV>(sc);
    [[maybe_unused]] const RT_CONST EnvRec *env = environment_of(sc.camera);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rays = 0, cast = 0, reached = 0;  // path searches, shadow searches, shadow rays that met nothing: this lane's, all samples
    if (k < a.count) {
        const Ray first = caller_ray(a.origin, a.direction, a.time, a.time_all, k);
        Xorwow rng = lane_stream(a, k);
        const bool media = (sc.flags & SCENE_HAS_MEDIA) != 0;
        Vec sum = mk(0.0, 0.0, 0.0);
        if (a.max_depth > 0) {  // otherwise no bounce runs: black, nothing drawn
            Ray ray = first;
            Vec carried = mk(1.0, 1.0, 1.0), acc = mk(0.0, 0.0, 0.0);  // thr and acc of include/rtow.h
            double sent = 0.0;                                         // q: the density the bounce before sent `ray` with
            int depth = 0, sample = 0;
            bool pending = false;  // a shadow ray (ray.o, shadow_d, ray.tm) up to shadow_end waits; where none is in the way it brings parked
            Vec shadow_d = mk(0.0, 0.0, 1.0), parked = mk(0.0, 0.0, 0.0);
            double shadow_end = 0.0;
            for (;;) {
                const bool shadow = pending;
                Ray searched = ray;
                double tmax = DBL_MAX;
                bool stop_at_first = false;
                if (shadow) {  // as shadow_kernel calls the search
                    searched.d = shadow_d;
                    tmax = shadow_end;
                    stop_at_first = !media;  // a medium's answer depends on what was found before it: the full search
                }
                HitInfo h;
                uint32_t leaf = kNone;
                const bool hit = query_search<T>(sc, d.node_leaf_pos, searched, 0.001, tmax, stop_at_first, h, leaf, rng);
                bool lamp = false, sampled = false, path_ends = false;
                [[maybe_unused]] bool sky = false, table = false;  // ENV: a miss weighted like a lamp end; the sample waits for the table's density
                [[maybe_unused]] double own = 0.0;                 // ENV: the density of a sky end or of an environment sample, this lane's alone
                // what the density loop and the fold behind it read: the ray the density is asked along, its light and weights
                Vec along_o = mk(0.0, 0.0, 0.0), along_d = mk(0.0, 0.0, 1.0), light = mk(0.0, 0.0, 0.0);
                double along_tm = 0.0, other = 0.0, distance = 0.0;
                if (shadow) {
                    cast++;
                    if (!hit) {
                        reached++;
                        acc = acc + parked;
                    }
                    pending = false;
                } else {
                    rays++;
                    Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
                    Vec normal;
                    uint32_t kind;
                    bool front;
                    const bool scattered = bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, true, true, normal, front, kind);
                    if (!scattered) {
                        path_ends = true;
                        lamp = hit && kind == MAT_DIFFUSE_LIGHT && sent > 0.0;
                        if constexpr (ENV) sky = !hit && sent > 0.0;
                        if (lamp) {  // weighted behind the density loop, along the incoming ray as given
                            along_o = ray.o;
                            along_d = ray.d;
                            along_tm = ray.tm;
                            light = carried * accumulated;
                            other = sent;
                        } else if (sky) {  // weighted against the environment sample the bounce before could have taken: no loop
                            own = environment_end_density(env, mcdf_lds, ray.d);
                            light = carried * accumulated;
                            other = sent;
                        } else {  // w = 1
                            acc = acc + carried * accumulated;
                        }
                    } else {
                        const Vec next = carried * throughput;
                        double sent_next = 0.0;
                        const bool sample_here = depth + 1 < a.max_depth;  // the last bounce takes none: its light sample would stand for bounce max_depth
                        if constexpr (ENV) {
                            if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && sample_here) {
                                sampled = path_emitter_sample<T>(sc, la, lds, env, mcdf_lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other,
                                                                 distance, sent_next, table, own);
                            }
                        } else if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && d.n_lights != 0 && sample_here) {
                            sampled = path_light_sample<T>(sc, la, lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other, distance, sent_next);
                        }
                        carried = next;
                        sent = sent_next;
                        if (++depth >= a.max_depth) path_ends = true;  // still alive after the last bounce: dropped (R/kernel.cu:71,97)
                    }
                }
                // every lane still in the loop is here again.  The mixture density along `along`, every such lane of the wave on the same
                // row (a lane that needs none runs the loop on a ray of its own that meets what it meets: its sum is not read)
                double density_sum = 0.0;
                if constexpr (ENV) {  // only the lanes that need the TABLE's density vote: a wave whose lanes all picked the sky skips the loop, and so does
                    // every wave where the table has no share (chance 1 beside lamps: c_l * sum is 0 without walking the table, a lamp end's w = q / q)
                    if (env->table_share != 0.0 && __ballot(lamp || table) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
                    density_sum = lamp || table ? env->table_share * density_sum : own;  // p of include/rtow.h, per emitter
                    lamp = lamp || sky;
                } else {
                    if (__ballot(lamp || sampled) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
                }
                if (lamp) {  // w = q / (q + p): the scattered ray found the lamp a light sample of the bounce before could have found
                    const double w = other / (other + density_sum);
                    acc = acc + w * light;
                }
                if (sampled) {  // w = p / (p + s); the shadow ray decides in this lane's next iteration
                    const double both = density_sum + other;
                    const double w = both == 0.0 ? 0.0 : density_sum / both;
                    parked = w * light;
                    shadow_d = along_d;
                    shadow_end = fmin(distance * (1.0 - 0x1p-20), DBL_MAX);
                    pending = true;
                }
                if (path_ends) {  // (never with a sample pending)
                    sum = sum + acc;
                    if (++sample >= a.samples) break;
                    ray = first;
                    carried = mk(1.0, 1.0, 1.0);
                    acc = mk(0.0, 0.0, 0.0);
                    sent = 0.0;
                    depth = 0;
                }
            }
        }
        if (a.radiance) {  // linear: the mean as rt_scene_radiance forms it
            const Vec mean = over(sum, (double)a.samples);
            store3(a.radiance, k, mean);
        }
        if (a.path_rays) a.path_rays[k] = rays;
        if (a.rng_out) store_stream(a.rng_out + (size_t)k * 6, 1, rng);
    }
    if (a.ray_counter) {  // three atomics per wave at the most: every lane of the wave is here again
        unsigned long long searched = rays, shadows = cast, unblocked = reached;
        for (int step = 32; step > 0; step >>= 1) {
            searched += __shfl_xor(searched, step, 64);
            shadows += __shfl_xor(shadows, step, 64);
            unblocked += __shfl_xor(unblocked, step, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
            if (searched) atomicAdd(a.ray_counter, searched);
            if (shadows) atomicAdd(d.shadow_counters, shadows);
            if (unblocked) atomicAdd(d.shadow_counters + 1, unblocked);
        }
    }
}

hipError_t RT_CAT(launch_radiance_direct_, RT_SUFFIX)(const DeviceScene &sc, const RadianceDirectArgs &d, hipStream_t stream, QueryKernelInfo *info)
{
    RT_TO_AFFINE(launch_radiance_direct_, sc, d, stream, info);
    const RadianceArgs &a = d.rad;
    if (a.samples < 1 || a.max_depth < 0 || !a.origin || !a.direction || !(a.radiance || a.path_rays || a.rng_out)) return hipErrorInvalidValue;
    if (!info && d.n_lights != 0 && (!d.rows || !d.cdf)) return hipErrorInvalidValue;
    if (!info && sc.world_kind == WORLD_BVH && !d.node_leaf_pos) return hipErrorInvalidValue;
    if (!info && a.ray_counter && !d.shadow_counters) return hipErrorInvalidValue;
    void (*kernel)(DeviceScene, RadianceDirectArgs) =
        sc.world_kind == WORLD_BVH ? radiance_direct_kernel<RT_STRICT, TBvhNested> : radiance_direct_kernel<RT_STRICT, TListNested>;
    if (sc.flags & SCENE_ENVIRONMENT_LIGHT)  // the instantiations that sample the environment too; every other scene launches what it did
        kernel = sc.world_kind == WORLD_BVH ? radiance_direct_kernel<RT_STRICT, TBvhNested, true> : radiance_direct_kernel<RT_STRICT, TListNested, true>;
    return info_or_launch(kernel, sc, d, a.count, stream, info);
}
#elif RT_FILM_DIRECT
// ------------------------------------------------------------------------------------------------
// Frames with light samples (rt_render_launch_direct; include/rtow.h states the operation): a film rendered by the estimator of
// rt_scene_radiance_direct.  The loop is radiance_direct_kernel's, restated line for line -- one world search an iteration, of the
// lane's path ray or of its pending shadow ray, the light sample and the mixture density between them, the light table staged in
// LDS once before the loop.  What is new is where the work comes from: the workgroups are persistent, and a lane without a pixel
// takes the next one from the film's queue word at the top of an iteration -- at the start of the kernel, and when its pixel has
// just finished -- with one atomic per wave (ballot, popcount, lane prefix).  Queue position q is pixel q % 64 of the 8x8 tile
// q / 64 of this rank's rows, numbered as render_kernel numbers them; a position outside the frame, or a pixel an adaptive frame
// has marked, is skipped by taking again.  A lane leaves when the queue is dry and it holds nothing; there is no barrier behind
// those of stage_lights, so lanes leave at different times.  One refinement, for the frame's last pixels: once the queue holds
// fewer positions than half the grid's lanes, a wave takes only when none of its lanes holds a pixel -- the last pixels
// then fill few waves, as a launch of a lane per pixel would fill them, instead of keeping every resident wave alive for one more
// pixel's time with a handful of lanes each (measured: profiles/r25_film_direct.txt).  A pixel is taken up and laid down as render_kernel does it (stream
// words, running sum, the planes of adaptive sampling), by one lane from its first sample to its last, from its own stream: the
// frame cannot depend on which lane took which pixel.
// ENV: as radiance_direct_kernel; the marginal table is staged once, before the persistent loop, like the light table.
// Termination: the queue word only grows, and a wave that has seen it pass the queue's length never takes again; a pixel is at
// most spp samples of at most max_depth path searches and as many shadow searches, each bounded as in radiance_direct_kernel
// (the two bisections of an environment sample each halve hi - lo).
// ------------------------------------------------------------------------------------------------
template <int STRICT, class T, bool ENV = false>
__global__ __launch_bounds__(256) void film_direct_kernel(DeviceScene sc, FilmDirectArgs d)
{
    __shared__ __attribute__((aligned(16))) double rows_lds[kLightLdsRows * kLightRowDoubles];
    __shared__ __attribute__((aligned(16))) double cdf_lds[kLightLdsRows];
    global_tables_only(sc);
    LightArgs la{};  // what the table's readers take
    la.rows = d.rows;
    la.cdf = d.cdf;
    la.n_lights = d.n_lights;
    stage_lights(la, rows_lds, cdf_lds);
    const LightLds lds{rows_lds, cdf_lds};
    [[maybe_unused]] const double *mcdf_lds = staged_environment<ENV>(sc);
    [[maybe_unused]] const RT_CONST EnvRec *env = environment_of(sc.camera);
    const CameraRec *__restrict__ cam = sc.camera;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tiles_x = ((uint32_t)d.width + 7u) >> 3;
    const uint32_t queue_len = tiles_x * (((uint32_t)d.rows_owned + 7u) >> 3) * 64u;
    const bool media = (sc.flags & SCENE_HAS_MEDIA) != 0;
    const bool adaptive = d.adaptive != 0;
    uint32_t rays = 0, cast = 0, reached = 0, taken = 0;  // path searches, shadow searches, shadow rays that met nothing, samples: this lane's, all its pixels
    bool dry = false;      // the queue word has passed the queue's length (the same for every lane of the wave still here)
    bool tail = false;     // the queue held fewer positions than half the grid's lanes when this wave last took (as uniform as dry)
    const uint32_t grid_lanes = gridDim.x * 256u;
    bool holding = false;  // this lane has a pixel
    // the pixel
    int i = 0, j = 0, sample = 0;
    size_t local = 0;
    Xorwow rng{};
    Vec col = mk(0.0, 0.0, 0.0);
    uint32_t ad_before = 0;
    double ad_q = 0.0;
    // the path: radiance_direct_kernel's state
    Ray ray;
    ray.o = mk(0.0, 0.0, 0.0);
    ray.d = mk(0.0, 0.0, 1.0);
    ray.tm = 0.0;
    Vec carried = mk(1.0, 1.0, 1.0), acc = mk(0.0, 0.0, 0.0);  // thr and acc of include/rtow.h
    double sent = 0.0;                                         // q: the density the bounce before sent `ray` with
    int depth = 0;
    bool pending = false;  // a shadow ray (ray.o, shadow_d, ray.tm) up to shadow_end waits; where none is in the way it brings parked
    Vec shadow_d = mk(0.0, 0.0, 1.0), parked = mk(0.0, 0.0, 0.0);
    double shadow_end = 0.0;
    for (;;) {
        // the take: every lane of the wave still in the loop is here.  One atomic for the lanes without a pixel, again while a
        // position fell outside the frame or on a marked pixel.
        while (!dry) {
            const unsigned long long here = __ballot(true);
            const unsigned long long need = __ballot(!holding);
            if (need == 0ull) break;
            if (tail && need != here) break;  // the last pixels: the wave waits until it is empty, then takes for all its lanes
            const uint32_t cnt = (uint32_t)__popcll(need);
            uint32_t base = 0;
            if (lane == (uint32_t)(__ffsll((long long)here) - 1)) base = atomicAdd(d.cursor, cnt);  // the first lane still here
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (base + cnt >= queue_len || base + cnt < base) dry = true;
            else tail = queue_len - (base + cnt) < grid_lanes / 2u;
            const uint32_t slot = base + (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
            if (!holding && slot >= base && slot < queue_len) {
                const uint32_t w = slot & 63u, tile = slot >> 6;
                const int pi = (int)((tile % tiles_x) * 8u + (w & 7u));
                const int lr = (int)((tile / tiles_x) * 8u + (w >> 3));
                bool take = pi < d.width && lr < d.rows_owned;
                if (take && adaptive) take = d.ad_mark[(size_t)lr * (size_t)d.width + (size_t)pi] == 0;  // stopped in an earlier launch of this frame: it stays as it is
                if (take) {
                    i = pi;
                    j = owned_row(lr, d.stripe_rows, d.rank, d.world_size);
                    local = (size_t)lr * (size_t)d.width + (size_t)pi;
                    if (adaptive) {
                        ad_before = d.ad_n[local];
                        ad_q = d.ad_q[local];
                    }
                    rng = load_stream(d.state + local, (size_t)d.n_pixels);
                    col = mk(0.0, 0.0, 0.0);
                    if (d.accum && d.spp_before > 0)  // progressive: continue the running sum in the same order
                        col = mk(d.accum[local * 3 + 0], d.accum[local * 3 + 1], d.accum[local * 3 + 2]);
                    sample = 0;
                    ray = camera_ray(cam, i, j, d.width, d.height, rng);
                    carried = mk(1.0, 1.0, 1.0);
                    acc = mk(0.0, 0.0, 0.0);
                    sent = 0.0;
                    depth = 0;
                    pending = false;
                    holding = true;
                }
            }
        }
        if (!holding) {
            if (dry) break;  // the queue is dry and this lane holds nothing
            continue;        // (the last pixels: lanes of this wave still hold theirs; it takes again when they are done)
        }
        bool lamp = false, sampled = false, path_ends = false;
        [[maybe_unused]] bool sky = false, table = false;  // ENV: a miss weighted like a lamp end; the sample waits for the table's density
        [[maybe_unused]] double own = 0.0;                 // ENV: the density of a sky end or of an environment sample, this lane's alone
        // what the density loop and the fold behind it read: the ray the density is asked along, its light and weights
        Vec along_o = mk(0.0, 0.0, 0.0), along_d = mk(0.0, 0.0, 1.0), light = mk(0.0, 0.0, 0.0);
        double along_tm = 0.0, other = 0.0, distance = 0.0;
        if (d.max_depth <= 0) {  // no bounce runs: black, only the camera's draws are taken
            path_ends = true;
        } else {
            const bool shadow = pending;
            Ray searched = ray;
            double tmax = DBL_MAX;
            bool stop_at_first = false;
            if (shadow) {  // as shadow_kernel calls the search
                searched.d = shadow_d;
                tmax = shadow_end;
                stop_at_first = !media;  // a medium's answer depends on what was found before it: the full search
            }
            HitInfo h;
            uint32_t leaf = kNone;
            const bool hit = query_search<T>(sc, d.node_leaf_pos, searched, 0.001, tmax, stop_at_first, h, leaf, rng);
            if (shadow) {
                cast++;
                if (!hit) {
                    reached++;
                    acc = acc + parked;
                }
                pending = false;
            } else {
                rays++;
                Vec throughput = mk(1.0, 1.0, 1.0), accumulated = mk(0.0, 0.0, 0.0);
                Vec normal;
                uint32_t kind;
                bool front;
                const bool scattered = bounce<T>(sc, ray, h, hit, rng, throughput, accumulated, true, true, normal, front, kind);
                if (!scattered) {
                    path_ends = true;
                    lamp = hit && kind == MAT_DIFFUSE_LIGHT && sent > 0.0;
                    if constexpr (ENV) sky = !hit && sent > 0.0;
                    if (lamp) {  // weighted behind the density loop, along the incoming ray as given
                        along_o = ray.o;
                        along_d = ray.d;
                        along_tm = ray.tm;
                        light = carried * accumulated;
                        other = sent;
                    } else if (sky) {  // weighted against the environment sample the bounce before could have taken: no loop
                        own = environment_end_density(env, mcdf_lds, ray.d);
                        light = carried * accumulated;
                        other = sent;
                    } else {  // w = 1
                        acc = acc + carried * accumulated;
                    }
                } else {
                    const Vec next = carried * throughput;
                    double sent_next = 0.0;
                    const bool sample_here = depth + 1 < d.max_depth;  // the last bounce takes none: its light sample would stand for bounce max_depth
                    if constexpr (ENV) {
                        if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && sample_here) {
                            sampled = path_emitter_sample<T>(sc, la, lds, env, mcdf_lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other,
                                                             distance, sent_next, table, own);
                        }
                    } else if ((kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) && d.n_lights != 0 && sample_here) {
                        sampled = path_light_sample<T>(sc, la, lds, ray, kind, normal, next, rng, along_o, along_d, along_tm, light, other, distance, sent_next);
                    }
                    carried = next;
                    sent = sent_next;
                    if (++depth >= d.max_depth) path_ends = true;  // still alive after the last bounce: dropped (R/kernel.cu:71,97)
                }
            }
        }
        // every lane that holds a pixel is here again.  The mixture density along `along`, every such lane of the wave on the same
        // row (a lane that needs none runs the loop on a ray of its own that meets what it meets: its sum is not read)
        double density_sum = 0.0;
        if constexpr (ENV) {  // only the lanes that need the TABLE's density vote: a wave whose lanes all picked the sky skips the loop, and so does
            // every wave where the table has no share (chance 1 beside lamps: c_l * sum is 0 without walking the table, a lamp end's w = q / q)
            if (env->table_share != 0.0 && __ballot(lamp || table) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
            density_sum = lamp || table ? env->table_share * density_sum : own;  // p of include/rtow.h, per emitter
            lamp = lamp || sky;
        } else {
            if (__ballot(lamp || sampled) != 0ull) density_sum = mixture_density(la, lds, along_o, along_d, along_tm);
        }
        if (lamp) {  // w = q / (q + p): the scattered ray found the lamp a light sample of the bounce before could have found
            const double w = other / (other + density_sum);
            acc = acc + w * light;
        }
        if (sampled) {  // w = p / (p + s); the shadow ray decides in this lane's next iteration
            const double both = density_sum + other;
            const double w = both == 0.0 ? 0.0 : density_sum / both;
            parked = w * light;
            shadow_d = along_d;
            shadow_end = fmin(distance * (1.0 - 0x1p-20), DBL_MAX);
            pending = true;
        }
        if (path_ends) {  // (never with a sample pending)  R/kernel.cu:143: col += RayColor(...)
            col = col + acc;
            taken++;
            bool more = ++sample < d.spp;
            bool converged = false;
            if (adaptive) {
                ad_q = adaptive_add_sample(ad_q, acc.x, acc.y, acc.z);
                // (also at the launch's cap: the mark must be right for a later launch of the frame)
                converged = adaptive_converged(d.rule, ad_before + (uint32_t)sample, col.x, col.y, col.z, ad_q);
                if (converged) more = false;
            }
            if (more) {
                ray = camera_ray(cam, i, j, d.width, d.height, rng);
                carried = mk(1.0, 1.0, 1.0);
                acc = mk(0.0, 0.0, 0.0);
                sent = 0.0;
                depth = 0;
            } else {
                // R/kernel.cu:146-153: save the RNG state, average, gamma 2
                store_stream(d.state + local, (size_t)d.n_pixels, rng);
                if (d.accum) {
                    d.accum[local * 3 + 0] = col.x;
                    d.accum[local * 3 + 1] = col.y;
                    d.accum[local * 3 + 2] = col.z;
                }
                if (adaptive) {  // the pixel's own n
                    const uint32_t n = ad_before + (uint32_t)sample;
                    d.ad_n[local] = n;
                    d.ad_q[local] = ad_q;
                    d.ad_mark[local] = converged ? 1 : 0;
                    col = over(col, (double)n);
                } else {
                    col = over(col, (double)(d.spp_before + d.spp));
                }
                d.pixels[local * 3 + 0] = sqrt(col.x);
                d.pixels[local * 3 + 1] = sqrt(col.y);
                d.pixels[local * 3 + 2] = sqrt(col.z);
                holding = false;
            }
        }
    }
    // four atomics per wave at the most: every lane of the wave is here again
    unsigned long long searched = rays, shadows = cast, unblocked = reached, samples = taken;
    for (int step = 32; step > 0; step >>= 1) {
        searched += __shfl_xor(searched, step, 64);
        shadows += __shfl_xor(shadows, step, 64);
        unblocked += __shfl_xor(unblocked, step, 64);
        samples += __shfl_xor(samples, step, 64);
    }
    if (lane == 0) {
        if (searched) atomicAdd(d.ray_counter, searched);
        if (adaptive && samples) atomicAdd(d.ray_counter + 2, samples);  // as the Adaptive<> render kernels count them
        if (shadows) atomicAdd(d.shadow_counters, shadows);
        if (unblocked) atomicAdd(d.shadow_counters + 1, unblocked);
    }
}

hipError_t RT_CAT(launch_film_direct_, RT_SUFFIX)(const DeviceScene &sc, const FilmDirectArgs &d, hipStream_t stream, FilmDirectInfo *info)
{
    RT_TO_AFFINE(launch_film_direct_, sc, d, stream, info);
    if (d.spp < 0 || d.max_depth < 0 || d.width <= 0 || d.rows_owned < 0) return hipErrorInvalidValue;
    if (!info) {
        if (!d.pixels || !d.state || !d.ray_counter || !d.cursor || !d.shadow_counters) return hipErrorInvalidValue;
        if (d.adaptive && (!d.ad_n || !d.ad_q || !d.ad_mark)) return hipErrorInvalidValue;
        if (d.n_lights != 0 && (!d.rows || !d.cdf)) return hipErrorInvalidValue;
        if (sc.world_kind == WORLD_BVH && !d.node_leaf_pos) return hipErrorInvalidValue;
    }
    const bool bvh = sc.world_kind == WORLD_BVH;
    void (*kernel)(DeviceScene, FilmDirectArgs) = bvh ? film_direct_kernel<RT_STRICT, TBvhNested> : film_direct_kernel<RT_STRICT, TListNested>;
    if (sc.flags & SCENE_ENVIRONMENT_LIGHT)  // the instantiations that sample the environment too; every other scene launches what it did
        kernel = bvh ? film_direct_kernel<RT_STRICT, TBvhNested, true> : film_direct_kernel<RT_STRICT, TListNested, true>;
    if (info) {
        hipFuncAttributes attr;
        if (hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(kernel)); e != hipSuccess) return e;
        info->kernel.vgprs = attr.numRegs;
        info->kernel.lds_bytes = (int)attr.sharedSizeBytes;
        info->kernel.kind = film_direct_kind(bvh ? props_of<TBvhNested>() : props_of<TListNested>(), d.adaptive != 0);
        info->scratch_bytes = (int)attr.localSizeBytes;
        return hipSuccess;
    }
    if (d.n_pixels == 0 || d.spp <= 0) return hipSuccess;
    int per_cu = 0;
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0); e != hipSuccess) return e;
    const uint32_t tiles = (((uint32_t)d.width + 7u) >> 3) * (((uint32_t)d.rows_owned + 7u) >> 3);
    const uint32_t blocks = film_direct_blocks(per_cu, d.max_blocks_per_cu, d.num_cus, tiles);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, sc, d);
    return hipGetLastError();
}
#elif RT_LANE_UNIT
// (a lane-per-ray unit defined above)
#elif RT_GROUP == 1
namespace {
template <bool AD>
hipError_t launch_composite_as(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info)
{
    using Any = std::conditional_t<AD, Adaptive<TListPrims>, TListPrims>;  // Like<Any, U>: U, adaptive or not
    switch (which) {
    case K_LIST_PRIMS: return launch_one<Like<Any, TListPrims>>(sc, a, stream, info);
    case K_LIST_INSTANCES: return launch_one<Like<Any, TListInstances>>(sc, a, stream, info);
    case K_LIST_INSTANCES_5:  // no adaptive form: choose_kernel gives adaptive frames the four-wave build
        if constexpr (AD) return hipErrorInvalidValue;
        else return launch_one<TListInstances5>(sc, a, stream, info);
    case K_LIST_PRIMS_GROUPED: return launch_one<Like<Any, TListPrimsGrouped>>(sc, a, stream, info);
    case K_LIST_INSTANCES_GROUPED: return launch_one<Like<Any, TListInstancesGrouped>>(sc, a, stream, info);
    case K_LIST_GENERAL: return launch_one<Like<Any, TListGeneral>>(sc, a, stream, info);
    case K_LIST_NESTED: return launch_one<Like<Any, TListNested>>(sc, a, stream, info);
    case K_BVH_INSTANCES: return launch_one<Like<Any, TBvhInstances>>(sc, a, stream, info);
    case K_BVH_MEDIA: return launch_one<Like<Any, TBvhMedia>>(sc, a, stream, info);
    case K_BVH_GENERAL: return launch_one<Like<Any, TBvhGeneral>>(sc, a, stream, info);
    case K_BVH_GENERAL_DEEP: return launch_one<Like<Any, TBvhGeneralDeep>>(sc, a, stream, info);
    case K_BVH_SEGMENTED: return launch_one<Like<Any, TBvhSegmented>>(sc, a, stream, info);
    case K_BVH_NESTED: return launch_one<Like<Any, TBvhNested>>(sc, a, stream, info);
    default: return hipErrorInvalidValue;
    }
}
} // namespace
#if RT_ADAPT
hipError_t RT_CAT(launch_adaptive_composite_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info)
{
    RT_TO_AFFINE(launch_adaptive_composite_, which, sc, a, stream, info);
    return launch_composite_as<true>(which, sc, a, stream, info);
}
#else
hipError_t RT_CAT(launch_composite_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info)
{
    RT_TO_AFFINE(launch_composite_, which, sc, a, stream, info);
    return launch_composite_as<false>(which, sc, a, stream, info);
}
#endif
#elif RT_ADAPT
// The rule exactly as this translation unit compiles it for its render kernels, on arrays: one more sample (ar, ag, ab) into q,
// then the rule on (n, r, g, b, q).  For the test that no build fuses the rule's operations (rt_adaptive_rule_on_device).
template <int STRICT>
__global__ __launch_bounds__(256) void adaptive_rule_kernel(AdaptiveRule rule, uint32_t count, const uint32_t *n, const double *sums_rgbq,
                                                            const double *sample_rgb, double *q_out, uint8_t *stops_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const double q = adaptive_add_sample(sums_rgbq[4 * (size_t)k + 3], sample_rgb[3 * (size_t)k], sample_rgb[3 * (size_t)k + 1], sample_rgb[3 * (size_t)k + 2]);
    q_out[k] = q;
    stops_out[k] = adaptive_converged(rule, n[k], sums_rgbq[4 * (size_t)k], sums_rgbq[4 * (size_t)k + 1], sums_rgbq[4 * (size_t)k + 2], q) ? 1 : 0;
}
hipError_t RT_CAT(launch_adaptive_rule_, RT_SUFFIX)(const AdaptiveRule &rule, uint32_t count, const uint32_t *n, const double *sums_rgbq,
                                                    const double *sample_rgb, double *q_out, uint8_t *stops_out, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_rule_kernel<RT_STRICT>, dim3((count + 255u) / 256u), dim3(256), 0, stream, rule, count, n, sums_rgbq, sample_rgb, q_out,
                       stops_out);
    return hipGetLastError();
}

hipError_t RT_CAT(launch_adaptive_prims_, RT_SUFFIX)(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info)
{
    switch (which) {
    case K_SPHERE_LIST: return launch_one<Adaptive<TSphereList>>(sc, a, stream, info);
    case K_BVH_PRIMS_FAST: return launch_one<Adaptive<TBvhPrimsFast>>(sc, a, stream, info);
    case K_BVH_PRIMS: return launch_one<Adaptive<TBvhPrims>>(sc, a, stream, info);
    default: return hipErrorInvalidValue;
    }
}
#else
namespace {
hipError_t launch_kernel(int which, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream, KernelInfo *info)
{
    // a film with adaptive sampling on: the same kernel among the Adaptive<> instantiations
    if (which >= K_FIRST_COMPOSITE)
        return a.adaptive ? RT_CAT(launch_adaptive_composite_, RT_SUFFIX)(which, sc, a, stream, info)
                          : RT_CAT(launch_composite_, RT_SUFFIX)(which, sc, a, stream, info);
    if (a.adaptive) return RT_CAT(launch_adaptive_prims_, RT_SUFFIX)(which, sc, a, stream, info);
    switch (which) {
    case K_SPHERE_LIST: return launch_one<TSphereList>(sc, a, stream, info);
    case K_BVH_PRIMS_FAST: return launch_one<TBvhPrimsFast>(sc, a, stream, info);
    case K_BVH_PRIMS: return launch_one<TBvhPrims>(sc, a, stream, info);
    default: return hipErrorInvalidValue;
    }
}
} // namespace

hipError_t RT_CAT(launch_render_, RT_SUFFIX)(int kernel, const DeviceScene &sc, const RenderArgs &a, hipStream_t stream)
{
    return launch_kernel(kernel, sc, a, stream, nullptr);
}

hipError_t RT_CAT(kernel_info_, RT_SUFFIX)(int kernel, const DeviceScene &sc, const RenderArgs &a, KernelInfo *info)
{
    return launch_kernel(kernel, sc, a, nullptr, info);
}
#endif

#if RT_MOVING
}  // namespace moving
#endif
} // namespace rtow

// An affine unit holds everything twice: once for the scenes whose chains hold static steps alone, once more with the moving step.
#if RT_AFFINE && !RT_MOVING
#undef RT_MOVING
#define RT_MOVING 1
#include "render.hip"
#endif
