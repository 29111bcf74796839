// scan_window_rule.h -- which trips of a RUN segment of the sphere-list scan (flat_scene.h ScanSegment) a ray can need, ONE
// definition: render.hip compiles it for the device (scan_filtered32), scene_builder.cpp for the host (rt_scene_dump_scan_windows,
// rt_scene_scan_window_trips; include/rtow.h).  Plain C++, no HIP include.
//
// The question.  The decided rows of a run (finite k) are spheres whose centres share one coordinate: they all lie in the SLAB
// slab_lo <= p[a] <= slab_hi, a the run's axis, slab_lo / slab_hi the least C[a] - r and the largest C[a] + r among them.  On a
// second axis w, the WINDOW axis, every trip of the run has a SPAN: the least C[w] - r and the largest C[w] + r among ITS decided
// rows.  Can the reference's Sphere::Hit accept the ray o + t d over (0.001, inf) for a decided row of trip T?  "No" must be a
// proof; "yes" may be wrong.
//
// The proof.  The reference accepts a root t > 0.001 of |o + t d - C|^2 = r^2 as it computes it.  The fp64 filter's comment in
// render.hip bounds what its rounding can do: disc / a differs from the exact r^2 - dist(line, C)^2 by less than 64 * 2^-53 W^2,
// W = |o| + |C| + r, and the accepted root, put back into the exact quadratic, leaves a residue of the same order.  So the point
// P = o + t d of an accepted hit has t > 0 and | |P - C|^2 - r^2 | < 2^-44 W^2, hence |P - C| < r + delta with
// delta = 2^-22 W (delta^2 alone is 2^-44 W^2).  P is a point of the ray with t >= 0 for which
//     slab_lo - delta <= P[a] <= slab_hi + delta      and      span_lo(T) - delta <= P[w] <= span_hi(T) + delta.
// The rule takes the part of {t >= 0} on which o[a] + t d[a] lies in [slab_lo - m, slab_hi + m] -- an interval [t0, t1], empty, or
// all of t >= 0 when d[a] = 0 and o[a] is inside -- and the extent [x0, x1] of o[w] + t d[w] over it: a linear function, so the
// extent is spanned by the two ends (the far end is -inf / +inf by the sign of d[w] where t1 is infinite, o[w] where d[w] = 0).
// Trip T is NEEDED when [x0 - m, x1 + m] meets [span_lo(T), span_hi(T)].  With m > delta plus every rounding below, P's t lies in
// [t0, t1], P[w] in [x0, x1], and the two intervals meet at P[w] give or take delta: a trip that is not needed holds no sphere
// the reference can accept.
//
// The margin.  W = |o| + reach with reach = DeviceScene::scan_reach32 (the decided rows' largest |C| + r: the same W as the
// filter's, render.hip scan_ray32), and m = 2^-16 W1 with W1 = |o.x| + |o.y| + |o.z| + reach, which needs no square root and lies
// between W and 1.74 W: a larger margin is still a margin.  Against m >= 2^-16 W stand
//   * delta = 2^-22 W, above;
//   * the host's roundings: slab and spans are formed in fp64 from the centres and sqrt(r2) and stored as fp32 numbers rounded
//     OUTWARDS (scene_builder.cpp build_scan_windows), so they only grow;
//   * the rule's arithmetic, fp64 with contraction off: t0, t1 carry three roundings each (a difference, the reciprocal's
//     division, a product), an end of the extent two more.  Where the exact end lies within 4 W of the origin, |t d[w]| <= 5 W and
//     the computed end is within 2^-48 W of it; where it lies farther out, the computed one is beyond 3 W, and every span lies
//     inside [-W, W]: on which side of a span the end falls is the same for both;
//   * the union of a wave's extents is held in fp32 (render.hip): 2^-24 of an end, at most 2^-22 W within 4 W, and beyond that
//     the end stays beyond 3 W as before.
// Together under 2^-21 W, a thirty-second of m.  C2: W = 30, m = 4.6e-4 to 8e-4, against cells a unit wide.
// A ray scan_ray32 calls degenerate (`sane` false: a = d.d outside (1e-280, 1e280), or W >= 1e15; here W1 >= 1e15, which is the
// case whenever W >= 1e15) needs every trip, and so does a
// ray for which anything here comes out NaN (d[a] so small that the reciprocal overflows, say): the last comparison is written so
// that a NaN answers "everything".
// Special rows need no flag: a trip that holds an undecided row (k = -inf) has the span (-inf, +inf) and meets every extent,
// the empty one included (the union of no ray is (+inf, -inf), and -inf <= -inf, +inf >= +inf hold); a trip of padding alone has
// the empty span (+inf, -inf) and meets only the extent that is everything.
#pragma once
#include <cstdint>

#include "flat_scene.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_WINDOW_FN __host__ __device__ inline
#else
#define RT_WINDOW_FN inline
#endif

namespace rtow {

// Which runs get a table (scene_builder.cpp build_scan_windows).  A window costs the wave about 150 vector instructions a pass --
// the extent of every lane, the wave's union, one test per trip, and two restarts of the row prefetch -- that is three trips' worth
// of the run form's 54.  What it can save is the trips outside the window: a wave's union is seldom narrower than a few spans, so
// with spans that each cover a quarter of the run's extent a window leaves out less than the few trips it costs.  A run gets a
// table when, on one of its two varying axes, the MEAN span of its trips (those with a finite span) is at most this fraction of
// the extent of all of them; the axis with the smallest mean wins (the lower axis on a tie).
constexpr double kScanWindowMaxMeanSpan = 0.25;

struct ScanExtent { double lo, hi; };  // (+inf, -inf): empty; (-inf, +inf): everything

// The extent on the window axis, margin included, of the part of the ray inside the slab.  oa, da / ow, dw: the ray's origin and
// direction on the slab's axis / on the window axis; o1 = |o.x| + |o.y| + |o.z|, a = d.d, reach = DeviceScene::scan_reach32.
RT_WINDOW_FN ScanExtent scan_window_extent(double oa, double da, double ow, double dw, double o1, double a, double reach, double slab_lo, double slab_hi)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double inf = __builtin_inf();
    const double w = o1 + reach;
    const bool sane = a > 1e-280 && a < 1e280 && w < 1e15;  // false wherever render.hip scan_ray32's is
    if (!sane) return ScanExtent{-inf, inf};
    const double m = 0x1p-16 * w;
    const double lo = slab_lo - m, hi = slab_hi + m;
    double xa, xb;
    if (da == 0.0) {
        if (!(oa >= lo && oa <= hi)) return ScanExtent{inf, -inf};
        xa = ow;
        xb = dw == 0.0 ? ow : (dw > 0.0 ? inf : -inf);
    } else {
        const double inv = 1.0 / da;
        const double ta = (lo - oa) * inv, tb = (hi - oa) * inv;
        double t0 = ta < tb ? ta : tb;
        const double t1 = ta < tb ? tb : ta;
        if (t1 < 0.0) return ScanExtent{inf, -inf};
        t0 = t0 > 0.0 ? t0 : 0.0;
        xa = ow + t0 * dw;
        xb = ow + t1 * dw;
    }
    const double x0 = (xa < xb ? xa : xb) - m, x1 = (xa < xb ? xb : xa) + m;
    if (!(x0 <= x1)) return ScanExtent{-inf, inf};  // a NaN anywhere (ta, tb, an end): everything
    return ScanExtent{x0, x1};
}

// Does a trip with this span have to run for rays whose extents unite to [x0, x1]?  (fp32 on both sides: the union as the wave holds it.)
RT_WINDOW_FN bool scan_window_needs(float span_lo, float span_hi, float x0, float x1) { return span_lo <= x1 && span_hi >= x0; }

// The trips to run out of one chunk's ballot of needed trips: gaps of one or two trips between needed ones are filled -- a jump
// costs the wave a restart of the row prefetch, about what two quiet trips cost.  Only bits between two set bits are added.
RT_WINDOW_FN unsigned long long scan_window_fill(unsigned long long need)
{
    const unsigned long long one = (need << 1) & (need >> 1);
    const unsigned long long two = ((need << 1) & (need >> 2)) | ((need << 2) & (need >> 1));
    return need | one | two;
}

} // namespace rtow
