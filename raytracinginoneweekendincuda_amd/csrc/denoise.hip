// denoise.hip -- one level of the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a full frame, gfx950.
//
// The stencil, as include/rtow.h rt_denoise_params states it: for pixel p and the 25 taps q = p + step * (dx, dy), dy outer, dx
// inner, both ascending, taps outside the frame skipped,
//     e = |c_p - c_q|^2 / sigma_color_k^2 + |a_p - a_q|^2 / sigma_albedo^2 + |n_p - n_q|^2 / sigma_normal^2
//         + ((z_p - z_q) / max(z_p, z_q, 1e-30))^2 / sigma_depth^2
//     w = h[dx + 2] * h[dy + 2] * exp(-e),   out_p = (sum w c_q) / (sum w),   h = {1/16, 1/4, 3/8, 1/4, 1/16}
// fp64 throughout, one exp per tap on the summed exponent, compiled without contraction.  The four 1 / sigma^2 come in as
// factors (AtrousArgs): a sigma of +inf is the factor 0 and its term an exact 0.  A tap whose colour is not finite is left out
// (weight 0); a centre whose colour is not finite passes through unchanged.
//
// One lane per pixel, 16 x 16 pixels per workgroup, every tap read straight from the planes: a 1200 x 800 frame and its guides
// are 77 MB and stay in the Infinity Cache (DESIGN.md section 5 has the measurement).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "render_iface.h"

namespace rtow {
namespace {

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 load3(const double *plane, size_t pixel) { return V3{plane[pixel * 3], plane[pixel * 3 + 1], plane[pixel * 3 + 2]}; }
__device__ __forceinline__ double dist_sq(V3 a, V3 b)
{
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

__global__ __launch_bounds__(256) void atrous_kernel(AtrousArgs a)
{
    const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const V3 cp = load3(a.in, p);
    if (!finite3(cp)) {
        a.out[p * 3] = cp.x;
        a.out[p * 3 + 1] = cp.y;
        a.out[p * 3 + 2] = cp.z;
        return;
    }
    V3 ap{0.0, 0.0, 0.0}, np{0.0, 0.0, 0.0};
    double zp = 0.0;
    if (a.albedo) ap = load3(a.albedo, p);
    if (a.normal) np = load3(a.normal, p);
    if (a.depth) zp = a.depth[p];
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    V3 sum{0.0, 0.0, 0.0};
    double wsum = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * a.step;
        if (qy < 0 || qy >= a.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * a.step;
            if (qx < 0 || qx >= a.width) continue;
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const V3 cq = load3(a.in, q);
            if (!finite3(cq)) continue;
            double e = dist_sq(cp, cq) * a.inv_color;
            if (a.albedo) e += dist_sq(ap, load3(a.albedo, q)) * a.inv_albedo;
            if (a.normal) e += dist_sq(np, load3(a.normal, q)) * a.inv_normal;
            if (a.depth) {
                const double zq = a.depth[q];
                const double r = (zp - zq) / fmax(fmax(zp, zq), 1e-30);
                e += (r * r) * a.inv_depth;
            }
            const double w = (h[dx + 2] * h[dy + 2]) * exp(-e);
            sum.x += w * cq.x;
            sum.y += w * cq.y;
            sum.z += w * cq.z;
            wsum += w;
        }
    }
    a.out[p * 3] = sum.x / wsum;
    a.out[p * 3 + 1] = sum.y / wsum;
    a.out[p * 3 + 2] = sum.z / wsum;
}

}  // namespace

hipError_t launch_atrous(const AtrousArgs &a, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid(((uint32_t)a.width + 15u) / 16u, ((uint32_t)a.height + 15u) / 16u), block(256);
    hipLaunchKernelGGL(atrous_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtow
