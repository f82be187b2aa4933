// Training on whole frames for gfx950 (MI355X): the stratified pair draw over a labelled scene cloud and the per-pair targets of
// utils/dataset.py:27-60 for MANY instances in one pass.  C ABI and the definitions: include/cppf.h ("Scene training"); host side:
// cppf_amd/scene_training.py; restated in numpy: tests/scene_training_ref.py.
//   st_draw_kernel      one lane per pair: one Philox block (stream 4), then either two gathers through the member list (a point of
//                       the target category, then a point of the SAME instance) or cppf_sample_pairs' uniform rule
//   st_targets_kernel   one lane per pair, workgroups of 256: the instance table (<= 32 rows of 12 floats + a flag word, < 2 KB) is
//                       staged in LDS once per workgroup; a lane gathers its two points, their labels and point a's normal (the only
//                       irregular traffic), does generate_target's arithmetic in fp32 and stores 4 + 16 + 2 + 1 + 4 bytes: `low` as
//                       one 32-bit word, `w_low` as one 128-bit word.  Up to four acosf per pair: whether the kernel is bound by
//                       them or by the gathers is a measurement (scripts/bench_scene_targets.py), not a claim.
// No atomics, no host synchronisation, no allocation: both calls can be captured in a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cppf.h"
#include "cppf_math.h"

#define ST_BLOCK 256
#define ST_MAX_K CPPF_SCENE_TRAIN_MAX_INSTANCES
#define ST_STREAM 4u                     // Philox counter word 2; 0 and 1 are cppf_sample_pairs', 2 and 3 the mesh statistics'

__global__ __launch_bounds__(ST_BLOCK) void st_draw_kernel(const int32_t* __restrict__ members, int members_cap,
                                                           const int32_t* __restrict__ seg_off, int n_inst, const int32_t* __restrict__ inst, uint32_t n_points,
                                                           int64_t n_pairs, int64_t n_pos_pairs, uint2 key, int2* __restrict__ idx)
{
    const int64_t p = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    const uint4 w = philox4x32_10(make_uint4((unsigned)p, 0u, ST_STREAM, 0u), key);
    int a = (int)(((unsigned long long)w.x * n_points) >> 32);
    int b = (int)(((unsigned long long)w.y * n_points) >> 32);
    const int M = seg_off[n_inst];
    if (p < n_pos_pairs && M > 0 && M <= members_cap) {
        // a list that does not keep its promises (more members than the buffer holds, a member outside the cloud, a label without a
        // segment, offsets that leave [0, M]) never makes this lane read outside members / inst: such a pair keeps the uniform draw
        const int am = members[(int)(((unsigned long long)w.x * (unsigned)M) >> 32)];
        if ((unsigned)am < n_points) {
            const int k = inst[am];
            if ((unsigned)k < (unsigned)n_inst) {
                const int s0 = seg_off[k], s1 = seg_off[k + 1];
                if (s0 >= 0 && s1 > s0 && s1 <= M) {
                    a = am;
                    b = members[s0 + (int)(((unsigned long long)w.y * (unsigned)(s1 - s0)) >> 32)];
                }
            }
        }
    }
    idx[p] = make_int2(a, b);
}

// value in [0, max] -> the lower of its two neighbouring bins and that bin's weight (training.real2prob's compact form)
__device__ __forceinline__ void st_bin(float v, float interval, int bins, int& low, float& w)
{
    const float x = v / interval;
    const int f = (int)floorf(x);
    low = f < bins - 2 ? f : bins - 2;
    w = 1.0f - (x - (float)low);
}

__device__ __forceinline__ float st_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(ST_BLOCK) void st_targets_kernel(const float* __restrict__ pc, const float* __restrict__ nrm,
                                                              const int32_t* __restrict__ inst, int n_points, const int2* __restrict__ idx,
                                                              int64_t n_pairs, const float* __restrict__ table,
                                                              const int32_t* __restrict__ flags, int n_inst, float v0, float v0x2, float v1,
                                                              float int_mu, float int_nu, float int_rot, int tr_bins, int rot_bins,
                                                              uint8_t* __restrict__ kind, int32_t* __restrict__ pair_inst,
                                                              uint32_t* __restrict__ low, float4* __restrict__ w_low, uint16_t* __restrict__ aux)
{
    __shared__ float s_tab[ST_MAX_K * 12];
    __shared__ int s_flag[ST_MAX_K];
    for (int t = threadIdx.x; t < n_inst * 12; t += ST_BLOCK) s_tab[t] = table[t];
    if ((int)threadIdx.x < n_inst) s_flag[threadIdx.x] = flags[threadIdx.x];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    const int2 ij = idx[p];
    // a negative pair: all nu weight on the farthest bin, the other heads on bin 0 (the loss ignores them)
    uint32_t lo_w = (uint32_t)(tr_bins - 2) << 8;
    float4 wl = make_float4(1.f, 0.f, 1.f, 1.f);
    uint16_t ax = 0;
    uint8_t kd = 0;
    int32_t pi = -1;
    if ((unsigned)ij.x >= (unsigned)n_points || (unsigned)ij.y >= (unsigned)n_points) {
        kd = 255;
    } else {
        const int k = inst[ij.x];
        if ((unsigned)k < (unsigned)n_inst && inst[ij.y] == k && (s_flag[k] & 1)) {
            using namespace cppf;
            const float* r = s_tab + 12 * k;
            const f3 c = {r[0], r[1], r[2]}, up = {r[3], r[4], r[5]}, right = {r[6], r[7], r[8]};
            const f3 a = sub3(ld3(pc, ij.x), c), b = sub3(ld3(pc, ij.y), c);
            const f3 d = sub3(a, b);
            const float len = sqrtf(dot3(d, d)) + 1e-7f;
            const f3 u = div3(d, len);
            const float proj = dot3(a, u);
            const f3 o = sub3(a, scl3(u, proj));
            const float dist2o = sqrtf(dot3(o, o));
            const float cu = dot3(u, up), cr = dot3(u, right);
            f3 n = ld3(nrm, ij.x);
            if (dot3(n, u) < 0.f) n = neg3(n);
            const float nu_ = dot3(n, up), nr_ = dot3(n, right);
            const float fin = ((proj + dist2o) + (cu + cr)) + (nu_ + nr_);         // finite iff all six are (a sum cannot undo an inf)
            if (isfinite(fin) && isfinite(proj) && isfinite(dist2o)) {
                float th_up = acosf(st_clamp(cu, -1.f, 1.f));
                if (s_flag[k] & 2) th_up = fminf(th_up, acosf(st_clamp(-cu, -1.f, 1.f)));
                float th_r = acosf(st_clamp(cr, -1.f, 1.f));
                if (s_flag[k] & 4) th_r = fminf(th_r, acosf(st_clamp(-cr, -1.f, 1.f)));
                int l0, l1, l2, l3;
                st_bin(st_clamp(proj + v0, 0.f, v0x2), int_mu, tr_bins, l0, wl.x);
                st_bin(st_clamp(dist2o, 0.f, v1), int_nu, tr_bins, l1, wl.y);
                st_bin(th_up, int_rot, rot_bins, l2, wl.z);
                st_bin(th_r, int_rot, rot_bins, l3, wl.w);
                lo_w = (uint32_t)l0 | ((uint32_t)l1 << 8) | ((uint32_t)l2 << 16) | ((uint32_t)l3 << 24);
                ax = (uint16_t)((nu_ > 0.f ? 1u : 0u) | (nr_ > 0.f ? 0x100u : 0u));
                kd = 1;
                pi = k;
            }
        }
    }
    kind[p] = kd;
    pair_inst[p] = pi;
    low[p] = lo_w;
    w_low[p] = wl;
    aux[p] = ax;
}

extern "C" int cppf_sample_scene_pairs(const int32_t* members, int64_t members_capacity, const int32_t* seg_off, int n_inst,
                                       const int32_t* inst, int64_t n_points, int64_t n_pairs, int64_t n_pos_pairs, unsigned long long seed,
                                       int32_t* idx, void* stream)
{
    if (n_pairs < 0 || n_pairs > INT32_MAX || n_pos_pairs < 0 || n_pos_pairs > n_pairs) return CPPF_EINVAL;
    if (n_pairs == 0) return 0;
    if (n_inst < 1 || n_points < 1 || n_points > INT32_MAX || !seg_off || !inst || !idx) return CPPF_EINVAL;
    if (members_capacity < 0 || members_capacity > INT32_MAX || (members_capacity > 0 && !members)) return CPPF_EINVAL;
    if ((uintptr_t)idx & 7u) return CPPF_EINVAL;                               // a pair is stored as one 8-byte word
    const unsigned blocks = (unsigned)((n_pairs + ST_BLOCK - 1) / ST_BLOCK);
    hipLaunchKernelGGL(st_draw_kernel, dim3(blocks), dim3(ST_BLOCK), 0, (hipStream_t)stream, members, (int)members_capacity, seg_off, n_inst,
                       inst, (uint32_t)n_points, n_pairs, n_pos_pairs, make_uint2((unsigned)seed, (unsigned)(seed >> 32)), (int2*)idx);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}

extern "C" int cppf_scene_pair_targets(const float* pc, const float* nrm, const int32_t* inst, int64_t n_points, const int32_t* idx,
                                       int64_t n_pairs, const float* table, const int32_t* flags, int n_inst, double vote_range0,
                                       double vote_range1, int tr_bins, int rot_bins, uint8_t* kind, int32_t* pair_inst, uint8_t* low,
                                       float* w_low, uint8_t* aux, void* stream)
{
    if (n_inst < 1 || n_inst > ST_MAX_K || n_pairs < 0 || n_pairs > INT32_MAX) return CPPF_EINVAL;
    if (tr_bins < 2 || tr_bins > 256 || rot_bins < 2 || rot_bins > 256) return CPPF_EINVAL;      // a bin index is one byte
    if (!(vote_range0 > 0.0) || !(vote_range1 > 0.0)) return CPPF_EINVAL;
    if (n_pairs == 0) return 0;
    if (n_points < 1 || n_points > INT32_MAX || !pc || !nrm || !inst || !idx || !table || !flags) return CPPF_EINVAL;
    if (!kind || !pair_inst || !low || !w_low || !aux) return CPPF_EINVAL;
    if (((uintptr_t)idx & 7u) || ((uintptr_t)low & 3u) || ((uintptr_t)w_low & 15u) || ((uintptr_t)aux & 1u)) return CPPF_EINVAL;
    // training.targets' constants, rounded to fp32 where torch rounds them: v0, 2 v0, v1 and the three bin widths (fp64, then once)
    const float v0 = (float)vote_range0, v0x2 = (float)(2.0 * vote_range0), v1 = (float)vote_range1;
    const float int_mu = (float)(2.0 * vote_range0 / (double)(tr_bins - 1)), int_nu = (float)(vote_range1 / (double)(tr_bins - 1));
    const float int_rot = (float)(3.141592653589793 / (double)(rot_bins - 1));
    const unsigned blocks = (unsigned)((n_pairs + ST_BLOCK - 1) / ST_BLOCK);
    hipLaunchKernelGGL(st_targets_kernel, dim3(blocks), dim3(ST_BLOCK), 0, (hipStream_t)stream, pc, nrm, inst, (int)n_points,
                       (const int2*)idx, n_pairs, table, flags, n_inst, v0, v0x2, v1, int_mu, int_nu, int_rot, tr_bins, rot_bins, kind,
                       pair_inst, (uint32_t*)low, (float4*)w_low, (uint16_t*)aux);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}
