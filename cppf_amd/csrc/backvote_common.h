// The back-vote's arithmetic (reference: CUDA backvote, models/voting.py:74-112), shared by backvote_body (pose_tail.hip: one
// centre; offsets / mask / chunk counts out) and backvote_multi_kernel (scene_multi.hip: up to 32 centres, one bit each).  Both
// run two stages per wave: stage 1, one pair per lane, screens out what cannot pass :101 for any rotation and queues the rest
// in LDS; stage 2 runs the queued rotation loops 64 at a time over the arc of bv_arc.  The kernels keep what differs: their
// loads, drain loops, survivor bookkeeping -- and their copies of the stage-1 screens (see backvote_body).
// Arguments and results go by value, in at most 16 registers per call: a reference or a wider list keeps the caller's variable
// in memory until the call is inlined, and backvote_kernel (the timed chain) then compiles to other code than it did before
// these functions were taken out of it.
#pragma once
#include "vote_common.h"

// ----------------------------------------------------------------------------- host: launch geometry
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
// blocks of 256 lanes for a grid-stride loop over n items: 1 .. 16384
static inline int blocks256(int64_t n) { return (int)((n + 255) / 256 < 16384 ? ((n + 255) / 256 > 0 ? (n + 255) / 256 : 1) : 16384); }
// blocks of a back-vote over n_ppfs pairs: BV_U = 4 pairs per thread and trip, 256 threads
static inline int64_t backvote_blocks(int64_t n_ppfs, int64_t cap = 1024)
{
    const int64_t nb = (n_ppfs + 4 * 256 - 1) / (4 * 256);
    return nb > cap ? cap : nb;
}
// LDS of a back-vote block: (cos, sin) table of every n <= n_rots (when it fits) | per-wave queues, 4 x 128 words | extra
static inline size_t backvote_lds_bytes(int n_rots, size_t extra = 0)
{
    const int entries = tri(n_rots);
    return (entries <= VOTE_TAB_LDS_MAX ? (size_t)entries * sizeof(float2) : 0) + 4 * 128 * sizeof(uint32_t) + extra;
}

// ----------------------------------------------------------------------------- rotation table
// The vote that produced the centre left the same table in its workspace (VOTE_TAB_STAMP): 21 KB to load instead of 2 628 fp64
// sincos per block.  The caller synchronises.
__device__ __forceinline__ void bv_load_rot_table(float2* ltab, int entries, int n_rots, const unsigned long long* __restrict__ vote_ws)
{
    const float2* wtab = reinterpret_cast<const float2*>(reinterpret_cast<const char*>(vote_ws) + VOTE_WS_TAB);
    if (vote_ws && vote_ws[31] == (VOTE_TAB_STAMP ^ (unsigned long long)n_rots) && rot_table_intact(wtab, n_rots)) {
        for (int e = threadIdx.x; e < entries; e += blockDim.x) ltab[e] = wtab[e];
    } else {
        fill_rot_table(ltab, entries, threadIdx.x, blockDim.x);
    }
}

__device__ __forceinline__ int bv_rot_count(float odist, float res, int n_rots)      // :97
{
    return min((int)((double)(odist / res) * (2 * CPPF_PI)), n_rots);
}

// ----------------------------------------------------------------------------- wave queue
// the lanes with `pass` append `item` at `tail` (the queue's end) in lane order; returns how many did
__device__ __forceinline__ int bv_push(uint32_t* tail, const bool pass, const uint32_t item)
{
    const unsigned long long m = __ballot(pass);
    if (pass) tail[__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0))] = item;
    return __popcll(m);
}

// ----------------------------------------------------------------------------- stage 2
// The reference's loop (:97-110) for one (pair, centre) that passed stage 1 runs over the ARC of rotations that can pass :101
// only, in index order: (lo, cnt) = rotations lo, lo + 1, .. modulo n, cnt of them.  With offset = cos(t) x + sin(t) y,
// |x| = |y| = rho and x, y, ab orthogonal,
//   |cc + offset - gt|^2 = |w|^2 + rho^2 - 2 (A cos t + B sin t),   w = gt - cc, A = w.x, B = w.y,
// so the distance test holds exactly where cos(t - phi) >= K / M, phi = atan2(B, A), M = |(A, B)|,
// K = (|w|^2 + rho^2 - tol^2) / 2: a run of indices around phi n / 2 pi, about 2 tol / res + 3 of them instead of n <= 72.
// The run is a superset (approximate acos / atan2 with their error bounds, one index of margin on either side, K lowered
// by the deviations of |offset|^2 from rho^2: roundings and the 1e-7 regulariser, which shortens ab by 1e-7 / L -- pairs
// closer than 1e-3, L2 = |a - b|^2 < 1e-6, scan everything); each candidate still goes through the reference's exact arithmetic
// and the first one in index order wins, so the result is the reference's.
// K is lowered once more for what the loop's OWN rounding does to :101.  The loop tests |fl(fl(cc + offset) - gt)| against tol:
// the sum is rounded at the size of the COORDINATES, half an ulp of up to cmax + rho per component (cmax = the largest |cc_i|),
// which moves the distance by up to sqrt(3) 2^-24 (cmax + rho) < dc = 2e-7 (cmax + rho) -- an absolute error that the terms
// relative to |w|, rho and tol above do not see: with a centre 8 away and tol = 6e-3 it is 1.5e-4 tol.  A sample whose exact
// distance is up to tol + dc can therefore pass, tol^2 may grow by (2 tol + dc) dc, and K goes down by (tol + dc) dc.  (Without
// this term the arc was empty for pairs whose one passing sample lay within 1e-4 tol of the cut, at |gt| = 8.5 and res <= 4e-3:
// tests/test_gpu_backvote_edges.py, 3 to 8 pairs of 13 888.)  On inputs where every pair survives stage 1 (a trained
// network) the full loop was the kernel: 100 us at C2, a lane walking on average 36 rotations and a wave its slowest lane's.
__device__ __forceinline__ int2 bv_arc(const float L2, const f3 w, const f3 x, const f3 y, const float tol, const int n, const float cmax)
{
    const float A_ = dot3(w, x), B_ = dot3(w, y), w2 = dot3(w, w), rho2 = dot3(x, x);
    int lo = 0, cnt = n;
    const float M = __builtin_amdgcn_sqrtf(A_ * A_ + B_ * B_);
    const float dc = 2e-7f * (cmax + __builtin_amdgcn_sqrtf(rho2));
    const float K = 0.5f * (w2 + rho2 - tol * tol) - (3e-4f * rho2 + 4e-6f * (w2 + rho2 + tol * tol) + (tol + dc) * dc);
    if (n > 0 && L2 >= 1e-6f && M > 1e-30f) {
        const float c = K * __builtin_amdgcn_rcpf(M);
        if (c > 1.0005f) {
            cnt = 0;                                   // no rotation comes within tol of the centre
        } else if (c > -0.9995f) {
            const float alpha = acos_approx(fminf(c, 1.f)) + 8e-4f;        // acos / atan2 errors, rcp, table angles
            const float phi = atan2_approx(B_, A_);
            const float k = (float)n * 0.159154943f;                       // n / 2 pi
            const float ic = phi * k, hw = fmaf(alpha, k, 1.0f);
            const int i_lo = (int)floorf(ic - hw), i_hi = (int)ceilf(ic + hw);
            if (i_hi - i_lo + 1 < n) {
                cnt = i_hi - i_lo + 1;
                lo = i_lo % n;
                lo = lo < 0 ? lo + n : lo;
            }
        }
    }
    return make_int2(lo, cnt);
}

// cmax of bv_arc: the largest coordinate of the circle's centre
__device__ __forceinline__ float bv_cmax(const f3 cc) { return fmaxf(fmaxf(fabsf(cc.x), fabsf(cc.y)), fabsf(cc.z)); }

// The two tests of one candidate rotation, pc = cc + offset: the reference's :101 and :103-107.  The first candidate in index
// order that passes both ends the loop (:109) with found = -offset (:108); a survivor (nocs/inference.py:230) has found != 0.
__device__ __forceinline__ bool bv_too_far(const f3 pc, const f3 gt, const float tol) { return len3(sub3(pc, gt)) > tol; }
__device__ __forceinline__ bool bv_outside(const f3 pc, const f3 cr, const float res, const float bx, const float by, const float bz)
{
    const f3 g = div3(sub3(pc, cr), res);
    return g.x < 0.f || g.y < 0.f || g.z < 0.f || g.x >= bx || g.y >= by || g.z >= bz;
}
