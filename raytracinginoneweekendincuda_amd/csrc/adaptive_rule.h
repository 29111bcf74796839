// adaptive_rule.h -- the stopping rule of adaptive sampling, ONE definition: render.hip compiles it for the device,
// device_scene.cpp for the host (rt_adaptive_converged, include/rtow.h).
//
// Per pixel the film keeps, next to the colour sum col = (r, g, b): n, the samples taken so far, and q, the sum of y^2 over
// those samples with y = (r_s + g_s) + b_s the plain sum of the three channels of sample s's radiance.  The rule is looked
// at exactly when n >= min_samples and (n - min_samples) % check_interval == 0, and the pixel stops at the first such n where
//
//     standard error of the mean of y  <=  noise_threshold * max(mean of y, luminance_floor)
//
// with the divisions and the square root multiplied out: (q - s^2 / N) / (N (N - 1)) <= tau^2 max(s / N, phi)^2 becomes
// q N - s^2 <= tau^2 (N - 1) max(s, phi N)^2.  The operations below are in the order include/rtow.h documents, and no build
// may contract them into fused multiply-adds: the device, the host and a restatement in any IEEE-754 double arithmetic then
// decide every pixel alike.  That is the pragma's job, and it needs a contraction mode that honours pragmas: the strict
// objects are built with -ffp-contract=off, the fast adaptive objects with -ffp-contract=fast-honor-pragmas (plain "fast" fuses
// in the backend whatever the pragma says: v_fma_f64 for q N - s^2), the host object that includes this header with the
// compiler's default, which honours it too (csrc/Makefile; tests/test_adaptive_gpu.py runs the rule of both device builds
// against numpy on sums an ulp from the threshold).
//
// This is the textbook rule, and it is known to stop too early where light is found rarely: a pixel whose first
// min_samples samples all miss the lamp of a Cornell box has q = s = 0 and "converges" through the luminance floor.
// min_samples is the user's guard against that; nothing here second-guesses it.  noise_threshold = 0 is accepted but not
// useful: for a pixel whose samples are all equal, q N - s^2 is rounding noise of either sign.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_RULE_FN __host__ __device__ inline
#else
#define RT_RULE_FN inline
#endif

namespace rtow {

struct AdaptiveRule {  // rt_adaptive_params, field for field
    int32_t min_samples, check_interval;
    double noise_threshold, luminance_floor;
};

// q after one more sample of radiance (r, g, b)
RT_RULE_FN double adaptive_add_sample(double q, double r, double g, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double y = (r + g) + b;
    const double yy = y * y;
    return q + yy;
}

// does a pixel with these sums stop at n?  (false below min_samples, off a check point, and wherever a NaN is involved)
RT_RULE_FN bool adaptive_converged(const AdaptiveRule &p, uint32_t n, double sum_r, double sum_g, double sum_b, double q)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (n < (uint32_t)p.min_samples) return false;
    if ((n - (uint32_t)p.min_samples) % (uint32_t)p.check_interval != 0u) return false;
    const double N = (double)n;
    const double s = (sum_r + sum_g) + sum_b;
    const double qn = q * N;
    const double ss = s * s;
    const double lhs = qn - ss;
    const double floor_n = p.luminance_floor * N;
    const double m = s > floor_n ? s : floor_n;  // max(s, phi N); a NaN s has already made lhs a NaN
    const double tt = p.noise_threshold * p.noise_threshold;
    const double rhs = (tt * (N - 1.0)) * (m * m);
    return lhs <= rhs;
}

} // namespace rtow
