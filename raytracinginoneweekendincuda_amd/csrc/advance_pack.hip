// advance_pack.hip -- the last two launches of a path advance (rt_scene_path_advance, rt_scene_path_advance_direct; render_iface.h
// AdvanceArgs, AdvanceDirectArgs), gfx950: the scan
// of the workgroups' survivor counts and the gather of the staged survivors into packed rows.  Neither depends on the scene or
// on the variant, so they are built once, here.
//
// The compaction is stable and no workgroup waits for another: advance_kernel (render.hip) leaves a flag per row and a count per
// workgroup, the scan below turns the counts into offsets (one workgroup, a loop whose bound the host knows), and the gather
// recomputes each workgroup's ballots from the flags.  The order between the three launches is the stream's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "render_iface.h"

namespace rtow {
namespace {

constexpr uint32_t kScanBlock = 1024;  // sixteen waves: 2^22 counts (a batch of 2^30 rows) are 4096 trips of the loop

// inclusive prefix over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, uint32_t lane)
{
    for (int step = 1; step < 64; step <<= 1) {
        const uint32_t below = __shfl_up(v, step, 64);
        if (lane >= (uint32_t)step) v += below;
    }
    return v;
}

// block_offsets[b] = block_counts[0] + ... + block_counts[b - 1]; *count_out = the sum of all n_blocks counts
__global__ __launch_bounds__(kScanBlock) void advance_scan_kernel(const uint32_t *block_counts, uint32_t *block_offsets, uint32_t n_blocks,
                                                                  uint32_t *count_out)
{
    __shared__ uint32_t wave_totals[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;  // the sum of every count before this trip's: the same in every thread
    for (uint32_t base = 0; base < n_blocks; base += kScanBlock) {  // (uniform bounds: every thread takes every barrier)
        const uint32_t b = base + threadIdx.x;
        const uint32_t mine = b < n_blocks ? block_counts[b] : 0u;
        const uint32_t inclusive = wave_inclusive(mine, lane);
        if (lane == 63) wave_totals[wave] = inclusive;
        __syncthreads();
        uint32_t before = 0, trip = 0;
        for (uint32_t w = 0; w < kScanBlock / 64; w++) {
            const uint32_t total = wave_totals[w];
            if (w < wave) before += total;
            trip += total;
        }
        if (b < n_blocks) block_offsets[b] = carry + before + (inclusive - mine);
        carry += trip;
        __syncthreads();  // wave_totals is written again by the next trip
    }
    if (threadIdx.x == 0) *count_out = carry;
}

template <class V>
__device__ __forceinline__ void move_row(const V *from, V *to, size_t k, size_t j, int width)
{
    for (int c = 0; c < width; c++) to[j * width + c] = from[k * width + c];
}

// One lane per row: survivor k goes to row j = block_offsets[its workgroup] + the survivors before it in the workgroup.  Every lane
// of the workgroup calls this (its only barrier); kNoRow for a lane that moves nothing.
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t packed_row(const AdvanceGatherArgs &a, uint32_t k, uint32_t *wave_survivors)
{
    const bool survivor = k < a.capacity && a.survivor[k] != 0;
    const unsigned long long ballot = __ballot(survivor);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_survivors[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (!survivor) return kNoRow;  // (behind the only barrier)
    uint32_t j = a.block_offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) j += wave_survivors[w];
    j += (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (j > k) return kNoRow;  // never: a row moves towards the front.  Nothing is written beyond the capacity whatever the flags hold
    return j;
}

__device__ __forceinline__ void move_rows(const AdvanceGatherArgs &a, uint32_t k, uint32_t j)
{
    if (a.to.origin) move_row(a.from.origin, a.to.origin, k, j, 3);
    if (a.to.direction) move_row(a.from.direction, a.to.direction, k, j, 3);
    if (a.to.time) a.to.time[j] = a.from.time[k];
    if (a.to.rng_state) move_row(a.from.rng_state, a.to.rng_state, k, j, 6);
    if (a.to.throughput) move_row(a.from.throughput, a.to.throughput, k, j, 3);
    if (a.to.ray_id) a.to.ray_id[j] = a.from.ray_id[k];
    if (a.to.t) a.to.t[j] = a.from.t[k];
    if (a.to.normal) move_row(a.from.normal, a.to.normal, k, j, 3);
    if (a.to.front_face) a.to.front_face[j] = a.from.front_face[k];
    if (a.to.material) a.to.material[j] = a.from.material[k];
}

__global__ __launch_bounds__(256) void advance_gather_kernel(AdvanceGatherArgs a)
{
    __shared__ uint32_t wave_survivors[4];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = packed_row(a, k, wave_survivors);
    if (j == kNoRow) return;
    move_rows(a, k, j);
}

// the same for an advance with light samples (rt_scene_path_advance_direct): the density the ray was sent with moves too
__global__ __launch_bounds__(256) void advance_direct_gather_kernel(AdvanceDirectGatherArgs a)
{
    __shared__ uint32_t wave_survivors[4];
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = packed_row(a.rows, k, wave_survivors);
    if (j == kNoRow) return;
    move_rows(a.rows, k, j);
    if (a.scatter_pdf_to) a.scatter_pdf_to[j] = a.scatter_pdf_from[k];
}

}  // namespace

hipError_t launch_advance_scan(const uint32_t *block_counts, uint32_t *block_offsets, uint32_t n_blocks, uint32_t *count_out, hipStream_t stream)
{
    if (!block_counts || !block_offsets || !count_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(advance_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, block_counts, block_offsets, n_blocks, count_out);
    return hipGetLastError();
}

hipError_t launch_advance_gather(const AdvanceGatherArgs &a, hipStream_t stream)
{
    if (!a.survivor || !a.block_offsets) return hipErrorInvalidValue;
    if (a.capacity == 0) return hipSuccess;
    hipLaunchKernelGGL(advance_gather_kernel, dim3((a.capacity + kAdvanceBlock - 1u) / kAdvanceBlock), dim3(kAdvanceBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_advance_direct_gather(const AdvanceDirectGatherArgs &a, hipStream_t stream)
{
    if (!a.rows.survivor || !a.rows.block_offsets || (a.scatter_pdf_to && !a.scatter_pdf_from)) return hipErrorInvalidValue;
    if (a.rows.capacity == 0) return hipSuccess;
    hipLaunchKernelGGL(advance_direct_gather_kernel, dim3((a.rows.capacity + kAdvanceBlock - 1u) / kAdvanceBlock), dim3(kAdvanceBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtow
