// Proposal verification for the mask-free scene paths on gfx950 (MI355X): per-proposal evidence from what the proposal stage has
// already computed (csrc/scene_multi.hip), for up to 32 proposals in one pass.  C ABI and the definitions: include/cppf.h
// ("Proposal verification"); host side: cppf_amd/scene_stage.py verify_proposals; restated in numpy: tests/verify_ref.py.
//   cppf_proposal_support   one pass over the pair list: per proposal k the pairs with both / exactly one endpoint in point mask k
//                           and how many of each survive the back-vote at centre k (bit k of surv_bits)
//   cppf_box_support        one pass over the cloud: per proposal k the members of mask k, the members inside the oriented box k and
//                           all points inside box k
// Both are bound by memory and gather latency.  The counters of a wavefront come from ballots and population counts (lane k keeps
// proposal k's), a workgroup adds them in LDS and issues one integer atomic per counter: the same words on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"

#define VF_MAX_K 32            // one bit per proposal in a 32-bit word (scene_multi.hip: BVM_MAX_CENTERS)
#define VF_MAX_PAIRS ((int64_t)1 << 27)   // cppf_backvote_multi's bound on the list that wrote surv_bits
#define VF_MAX_BLOCKS 1024     // 4 workgroups of 256 per CU; longer inputs take the grid-stride loop (tests/test_gpu_verify.py: a second trip)

static inline size_t vf_align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline unsigned vf_blocks(int64_t n) { const int64_t b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : (b < VF_MAX_BLOCKS ? b : VF_MAX_BLOCKS)); }

// member[n] bit k = point n is in mask k (a non-zero byte)
__global__ __launch_bounds__(256) void vf_fold_masks_kernel(const uint8_t* __restrict__ point_masks, int64_t n_points, int n_props,
                                                            uint32_t* __restrict__ member)
{
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < n_points; n += (int64_t)gridDim.x * blockDim.x) {
        uint32_t w = 0;
        for (int k = 0; k < n_props; ++k) w |= (point_masks[(int64_t)k * n_points + n] ? 1u : 0u) << k;
        member[n] = w;
    }
}

// the workgroup's end of both kernels: lane k < n_props of every wavefront holds NC counters of proposal k in mine[]; they are added
// in LDS and leave as one global atomic per counter
template <int NC>
__device__ __forceinline__ void vf_flush(int (&mine)[NC], int* lsum, int n_props, int32_t* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < NC * VF_MAX_K; e += blockDim.x) lsum[e] = 0;
    __syncthreads();
    if (lane < n_props) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (mine[c]) atomicAdd(lsum + lane * NC + c, mine[c]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NC * n_props; e += blockDim.x)
        if (lsum[e]) atomicAdd(counts + e, lsum[e]);
}

// counts[k] = {within, agree, cross, cross_agree}
__global__ __launch_bounds__(256) void vf_proposal_support_kernel(const int32_t* __restrict__ idx, const uint32_t* __restrict__ surv_bits,
                                                                  const uint32_t* __restrict__ member, int64_t n_pairs, int64_t n_points,
                                                                  int n_props, uint32_t k_mask, int32_t* __restrict__ counts)
{
    __shared__ int lsum[4 * VF_MAX_K];
    const int lane = threadIdx.x & 63;
    int mine[4] = {0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // (the loop bound is wave-uniform: lanes past the end carry zero words into the ballots)
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n_pairs; base += stride) {
        const int64_t p = base + lane;
        uint32_t within = 0, cross = 0, s = 0;
        if (p < n_pairs) {
            const int2 ij = reinterpret_cast<const int2*>(idx)[p];
            s = surv_bits[p] & k_mask;
            const uint32_t ma = (ij.x >= 0 && ij.x < n_points) ? member[ij.x] : 0u;
            const uint32_t mb = (ij.y >= 0 && ij.y < n_points) ? member[ij.y] : 0u;
            within = ma & mb;
            cross = ma ^ mb;
        }
        const uint32_t agree = within & s, cagree = cross & s;
        for (int k = 0; k < n_props; ++k) {
            const int c0 = __popcll(__ballot((within >> k) & 1u)), c1 = __popcll(__ballot((agree >> k) & 1u));
            const int c2 = __popcll(__ballot((cross >> k) & 1u)), c3 = __popcll(__ballot((cagree >> k) & 1u));
            if (lane == k) { mine[0] += c0; mine[1] += c1; mine[2] += c2; mine[3] += c3; }
        }
    }
    vf_flush<4>(mine, lsum, n_props, counts);
}

extern "C" size_t cppf_proposal_support_workspace_bytes(int64_t n_points)
{
    return n_points < 0 ? 0 : vf_align256((size_t)n_points * sizeof(uint32_t));
}

extern "C" int cppf_proposal_support(const int32_t* point_idxs, const uint32_t* surv_bits, const uint8_t* point_masks, int64_t n_pairs,
                                     int64_t n_points, int n_props, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_props < 1 || n_props > VF_MAX_K || n_points < 1 || n_points > INT32_MAX || n_pairs < 0 || n_pairs >= VF_MAX_PAIRS)
        return CPPF_EINVAL;
    if (!point_masks || !counts || (n_pairs > 0 && (!point_idxs || !surv_bits))) return CPPF_EINVAL;
    if (!workspace || workspace_bytes < cppf_proposal_support_workspace_bytes(n_points)) return CPPF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_props * 4 * sizeof(int32_t), st)) return (int)e;
    if (n_pairs == 0) return 0;
    uint32_t* member = static_cast<uint32_t*>(workspace);
    const uint32_t k_mask = n_props == 32 ? 0xffffffffu : ((1u << n_props) - 1u);
    hipLaunchKernelGGL(vf_fold_masks_kernel, dim3(vf_blocks(n_points)), dim3(256), 0, st, point_masks, n_points, n_props, member);
    hipLaunchKernelGGL(vf_proposal_support_kernel, dim3(vf_blocks(n_pairs)), dim3(256), 0, st, point_idxs, surv_bits, member, n_pairs,
                       n_points, n_props, k_mask, counts);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}

// counts[k] = {mask_pts, mask_in_box, box_pts}.  The inside test, fp32, for a = 0, 1, 2: |d.x A[0][a] + d.y A[1][a] + d.z A[2][a]| <=
// half[a] with d = p - c, the products summed left to right (-ffp-contract=off: no fused multiply-add).  A NaN anywhere compares false.
__global__ __launch_bounds__(256) void vf_box_support_kernel(const float* __restrict__ points, const uint8_t* __restrict__ point_masks,
                                                             const float* __restrict__ centers, const float* __restrict__ axes,
                                                             const float* __restrict__ half, int64_t n_points, int n_props,
                                                             int32_t* __restrict__ counts)
{
    __shared__ float box[VF_MAX_K * 15];       // per proposal: centre[3] | axes[9] | half[3]
    __shared__ int lsum[3 * VF_MAX_K];
    for (int e = threadIdx.x; e < n_props * 15; e += blockDim.x) {
        const int k = e / 15, j = e % 15;
        box[e] = j < 3 ? centers[3 * k + j] : (j < 12 ? axes[9 * k + (j - 3)] : half[3 * k + (j - 12)]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int mine[3] = {0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n_points; base += stride) {
        const int64_t n = base + lane;
        const bool live = n < n_points;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (live) { px = points[3 * n]; py = points[3 * n + 1]; pz = points[3 * n + 2]; }
        const bool finite = live && isfinite(px) && isfinite(py) && isfinite(pz);
        for (int k = 0; k < n_props; ++k) {      // wave-uniform: the box is a broadcast read
            const float* b = box + 15 * k;
            const float dx = px - b[0], dy = py - b[1], dz = pz - b[2];
            const float t0 = (dx * b[3] + dy * b[6]) + dz * b[9];
            const float t1 = (dx * b[4] + dy * b[7]) + dz * b[10];
            const float t2 = (dx * b[5] + dy * b[8]) + dz * b[11];
            const bool in = finite && fabsf(t0) <= b[12] && fabsf(t1) <= b[13] && fabsf(t2) <= b[14];
            const bool mem = live && point_masks[(int64_t)k * n_points + n] != 0;
            const int c0 = __popcll(__ballot(mem)), c1 = __popcll(__ballot(mem && in)), c2 = __popcll(__ballot(in));
            if (lane == k) { mine[0] += c0; mine[1] += c1; mine[2] += c2; }
        }
    }
    vf_flush<3>(mine, lsum, n_props, counts);
}

extern "C" int cppf_box_support(const float* points, const uint8_t* point_masks, const float* centers, const float* axes, const float* half,
                                int64_t n_points, int n_props, int32_t* counts, void* stream)
{
    if (n_props < 1 || n_props > VF_MAX_K || n_points < 1 || n_points > INT32_MAX) return CPPF_EINVAL;
    if (!points || !point_masks || !centers || !axes || !half || !counts) return CPPF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_props * 3 * sizeof(int32_t), st)) return (int)e;
    hipLaunchKernelGGL(vf_box_support_kernel, dim3(vf_blocks(n_points)), dim3(256), 0, st, points, point_masks, centers, axes, half,
                       n_points, n_props, counts);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}
