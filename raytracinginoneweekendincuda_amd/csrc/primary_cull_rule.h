// primary_cull_rule.h -- which spheres of a sphere list a CAMERA ray through an 8x8 tile of pixels can possibly hit, ONE
// definition: render.hip compiles it for the device (primary_lists_kernel), scene_builder.cpp for the host
// (rt_scene_dump_primary_lists, include/rtow.h).  Plain C++, no HIP include.
//
// The question.  camera_ray (render.hip; R/Camera.h:76-85) produces, for pixel (i, j) of a width x height frame,
//     o = origin + lens_radius (px u + py v),   px^2 + py^2 < 1
//     d = llc + s horizontal + t vertical - o,  s = fl32(i + xi) / width,  t = fl32(j + eta) / height,  xi, eta in (0, 1]
// (fl32(i + xi) lies in [i, i + 1]: both ends are fp32 numbers and rounding is monotone).  Can the reference's Sphere::Hit accept
// such a ray for a sphere (C, r) over (0.001, inf), for any pixel of the rectangle i0..i1 x j0..j1?  "No" must be a proof; "yes"
// may be wrong.
//
// The proof.  Write A = origin, and B = llc + sc horizontal + tc vertical for the centre (sc, tc) of the rectangle
// [(i0 - 1) / width, (i1 + 2) / width] x [(j0 - 1) / height, (j1 + 2) / height] -- the pixels' own rectangle, closed on both sides
// because the jitter reaches both ends, padded by a pixel on every side.  With hs, ht its half extents:
//   * o lies within rho_A = lens_radius * smax(u, v) of A, smax the largest singular value of the 3x2 matrix (u v)
//     (|px u + py v| <= smax |(px, py)|; 1 for the orthonormal pair a look-at camera has, but nothing here assumes that);
//   * o + d lies within rho_B = max(|hs horizontal + ht vertical|, |hs horizontal - ht vertical|) of B (a norm is convex: over
//     the rectangle |ds horizontal + dt vertical| is largest at a corner).
// The ray's point at parameter tau >= 0 is P = (1 - tau) o + tau (o + d); the axis point X(tau) = (1 - tau) A + tau B.  So
//     |P - X(tau)| <= |1 - tau| rho_A + tau rho_B <= rho_A + tau k,      k = rho_A + rho_B.
// The reference accepts only where its discriminant is positive, i.e. (up to its rounding, below) where the ray's LINE comes within r
// of C, and every accepted root is a tau > 0.001 > 0 with |P(tau) - C| = r up to rounding; it is enough that no point of the ray
// with tau >= 0 comes within r' of C (r' = r plus the margin below).  By the triangle inequality that holds when
//     |X(tau) - C| > q + k tau  for every tau >= 0,      q = r' + rho_A,
// and with w = A - C, m = B - A, both sides non-negative, that is  h(tau) = a2 tau^2 + 2 b1 tau + c0 > 0  for tau >= 0 with
//     a2 = m.m - k^2,   b1 = w.m - q k,   c0 = w.w - q^2.
// (This is the cone of the issue's sketch with the half angle the union of the balls really has, sin alpha = k / |m|: the set
// {dist_axis - sigma lambda <= rho_A} with sigma = k / |m| does not contain those balls, whose envelope is steeper.)
// For a2 > 0 the quadratic is positive on tau >= 0 exactly when c0 > 0 and (b1 >= 0 or c0 a2 > b1^2).  a2 <= 0 -- the rays of the
// tile fan out over more than a half space, a lens as large as the focus distance -- answers "yes".
// Nothing is assumed about where the camera is: a camera inside the sphere has c0 < 0 ("yes"), a sphere behind it has b1 > 0 and
// c0 > 0 ("no" when it is clear of the lens), lens_radius = 0 gives rho_A = 0.
//
// The margins.
//   * The reference's rounding.  The fp64 filter's comment in render.hip proves that the reference's disc, divided by a = d.d,
//     differs from the exact r^2 - dist(line, C)^2 by less than 64 * 2^-53 W^2, W = |o| + |C| + r.  So a sphere is accepted only if
//     its line distance is below sqrt(r^2 + 64 * 2^-53 W^2); the rule uses r'^2 = r2 + 2^-40 (|A| + rho_A + |C| + sqrt(r2))^2, 128
//     times that (r2 = fl(radius * radius), the number the reference's test itself uses; a negative radius has the same r2).
//   * The ray's own rounding.  o and d are computed in fp64 from the camera's vectors: each is within a few 2^-53 S of its exact
//     value, S = |A| + |llc| + |horizontal| + |vertical| + lens_radius (|u| + |v|).  rho_A and rho_B each get 2^-40 S on top, and
//     a further 2^-40 of themselves for their own evaluation.
//   * The rule's own arithmetic.  With Wc = |A| + |C| (which bounds |w| and every rounding of w's components), a2, b1 and c0 are each
//     sums of at most seven products, computed within 32 * 2^-53 of n2 = m.m + k^2, sqrt(n2 n0) and n0 = Wc^2 + q^2; c0 a2 and b1^2
//     are at most n0 n2 (Cauchy-Schwarz).  The rule asks for
//         a2 > 2^-40 n2,   c0 > 2^-40 n0,   and  b1 >= 0  or  c0 a2 - b1^2 > 2^-40 n0 n2,
//     2^8 times those errors; where a computed b1 >= 0 hides a true b1 of -32 * 2^-53 sqrt(n0 n2), the true b1^2 is 2^-96 n0 n2, far
//     below the c0 a2 > 2^-80 n0 n2 the first two conditions leave.
// Contraction is switched off for the rule (as in adaptive_rule.h), and the kernel that runs it is compiled once, in a strict
// object: host and device then build the same lists.  Were they to differ in a borderline sphere, both lists would still be
// supersets of what the reference can accept.
#pragma once
#include <cstdint>

#include "flat_scene.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_CULL_FN __host__ __device__ inline
#else
#define RT_CULL_FN inline
#endif

namespace rtow {

// A tile's list in device memory: 16 uint16 words = 32 bytes.  [0] = the number of listed spheres, or kPrimaryNoList: too many,
// the tile has no list and its camera rays go through the scan; [1 .. count] = positions in the sphere list, ascending.
constexpr uint32_t kPrimaryListWords = 16;
constexpr uint32_t kPrimaryListMax = 14;
constexpr uint32_t kPrimaryNoList = 15;

struct TilePixels {  // a rectangle of pixels in true frame coordinates, both ends included
    int32_t i0, i1, j0, j1;
};

// The pixels of tile `tile` (8x8, row-major over this rank's compact rows) of a film: columns clipped to the frame, rows the
// smallest and the largest true row among the tile's local rows (a stripe height that is no multiple of 8 makes the rectangle
// larger, never wrong).
RT_CULL_FN TilePixels primary_tile_pixels(uint32_t tile, int32_t width, int32_t rows_owned, int32_t stripe_rows, int32_t rank, int32_t world_size)
{
    const uint32_t tiles_x = ((uint32_t)width + 7u) >> 3;
    const int32_t tx = (int32_t)(tile % tiles_x), ty = (int32_t)(tile / tiles_x);
    TilePixels t;
    t.i0 = tx * 8;
    t.i1 = tx * 8 + 7 < width ? tx * 8 + 7 : width - 1;
    const int32_t lr0 = ty * 8, lr1 = ty * 8 + 7 < rows_owned ? ty * 8 + 7 : rows_owned - 1;
    t.j0 = 0x7fffffff;
    t.j1 = -1;
    for (int32_t lr = lr0; lr <= lr1; lr++) {
        const int32_t j = ((lr / stripe_rows) * world_size + rank) * stripe_rows + (lr % stripe_rows);  // render.hip owned_row
        t.j0 = j < t.j0 ? j : t.j0;
        t.j1 = j > t.j1 ? j : t.j1;
    }
    return t;
}

struct TileCone {      // what the rule needs of a tile, computed once per tile
    double ax, ay, az; // A, the lens centre
    double mx, my, mz; // m = B - A
    double rho_a, k;   // with their margins
    double mm, kk;     // m.m, k^2
    double a_norm;     // |A|
    bool open;         // a2 > 2^-40 n2: the rule can say "no" at all
};

RT_CULL_FN double cull_norm3(double x, double y, double z) { return __builtin_sqrt(x * x + y * y + z * z); }

RT_CULL_FN TileCone primary_tile_cone(const CameraRec &c, int32_t width, int32_t height, const TilePixels &t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s0 = (double)(t.i0 - 1) / (double)width, s1 = (double)(t.i1 + 2) / (double)width;
    const double t0 = (double)(t.j0 - 1) / (double)height, t1 = (double)(t.j1 + 2) / (double)height;
    const double sc = 0.5 * (s0 + s1), tc = 0.5 * (t0 + t1), hs = 0.5 * (s1 - s0), ht = 0.5 * (t1 - t0);
    TileCone k;
    k.ax = c.origin[0]; k.ay = c.origin[1]; k.az = c.origin[2];
    k.mx = c.llc[0] + sc * c.horizontal[0] + tc * c.vertical[0] - k.ax;
    k.my = c.llc[1] + sc * c.horizontal[1] + tc * c.vertical[1] - k.ay;
    k.mz = c.llc[2] + sc * c.horizontal[2] + tc * c.vertical[2] - k.az;
    const double uu = c.u[0] * c.u[0] + c.u[1] * c.u[1] + c.u[2] * c.u[2], vv = c.v[0] * c.v[0] + c.v[1] * c.v[1] + c.v[2] * c.v[2];
    const double uv = c.u[0] * c.v[0] + c.u[1] * c.v[1] + c.u[2] * c.v[2];
    const double smax = __builtin_sqrt(0.5 * ((uu + vv) + __builtin_sqrt((uu - vv) * (uu - vv) + 4.0 * (uv * uv))));
    const double lens = c.lens_radius < 0.0 ? -c.lens_radius : c.lens_radius;
    k.a_norm = cull_norm3(k.ax, k.ay, k.az);
    const double scale = k.a_norm + cull_norm3(c.llc[0], c.llc[1], c.llc[2]) + cull_norm3(c.horizontal[0], c.horizontal[1], c.horizontal[2]) +
                         cull_norm3(c.vertical[0], c.vertical[1], c.vertical[2]) + lens * (__builtin_sqrt(uu) + __builtin_sqrt(vv));
    const double slack = 0x1p-40 * scale;
    const double plus = cull_norm3(hs * c.horizontal[0] + ht * c.vertical[0], hs * c.horizontal[1] + ht * c.vertical[1], hs * c.horizontal[2] + ht * c.vertical[2]);
    const double minus = cull_norm3(hs * c.horizontal[0] - ht * c.vertical[0], hs * c.horizontal[1] - ht * c.vertical[1], hs * c.horizontal[2] - ht * c.vertical[2]);
    k.rho_a = (lens * smax) * (1.0 + 0x1p-40) + slack;
    const double rho_b = (plus > minus ? plus : minus) * (1.0 + 0x1p-40) + slack;
    k.k = k.rho_a + rho_b;
    k.mm = k.mx * k.mx + k.my * k.my + k.mz * k.mz;
    k.kk = k.k * k.k;
    k.open = k.mm - k.kk > 0x1p-40 * (k.mm + k.kk);  // (false for a NaN anywhere: every sphere is then listed)
    return k;
}

// Can a camera ray of the tile be accepted by the reference's test for the sphere (cx, cy, cz), r2 = radius^2?  false is a proof.
RT_CULL_FN bool primary_may_hit(const TileCone &k, double cx, double cy, double cz, double r2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!k.open) return true;
    const double c_norm = cull_norm3(cx, cy, cz);
    const double reach = k.a_norm + k.rho_a + c_norm + __builtin_sqrt(r2);
    const double q = __builtin_sqrt(r2 + 0x1p-40 * (reach * reach)) + k.rho_a;
    const double wx = k.ax - cx, wy = k.ay - cy, wz = k.az - cz;
    const double wc = k.a_norm + c_norm;
    const double n0 = wc * wc + q * q, n2 = k.mm + k.kk;
    const double c0 = (wx * wx + wy * wy + wz * wz) - q * q;
    const double b1 = (wx * k.mx + wy * k.my + wz * k.mz) - q * k.k;
    const double a2 = k.mm - k.kk;
    const bool clear = c0 > 0x1p-40 * n0 && (b1 >= 0.0 || c0 * a2 - b1 * b1 > 0x1p-40 * (n0 * n2));
    return !clear;  // (a NaN anywhere compares false: "yes")
}

// One tile's list from the whole sphere list (host form; the device kernel runs the same two functions over scalar row loads).
inline void primary_list_for_tile(const TileCone &k, const SphereGeom *spheres, uint32_t n_spheres, uint16_t out[kPrimaryListWords])
{
    for (uint32_t w = 0; w < kPrimaryListWords; w++) out[w] = 0;
    uint32_t count = 0;
    for (uint32_t s = 0; s < n_spheres && count <= kPrimaryListMax; s++) {
        if (!primary_may_hit(k, spheres[s].cx, spheres[s].cy, spheres[s].cz, spheres[s].r2)) continue;
        if (count < kPrimaryListMax) out[1 + count] = (uint16_t)s;
        count++;
    }
    if (count > kPrimaryListMax) {
        for (uint32_t w = 0; w < kPrimaryListWords; w++) out[w] = 0;
        count = kPrimaryNoList;
    }
    out[0] = (uint16_t)count;
}

} // namespace rtow
