// The per-proposal stage of the mask-free scene path for gfx950 (MI355X), all proposals in one pass over the pair list:
//   cppf_backvote_multi      the back-vote of models/voting.py:74-112 at up to 32 centres: bit k of surv_bits[p] = pair p survives
//                            at centres[k]
//   cppf_segment_instances   the "unsupervised instance segmentation" of nocs/zero_shot.ipynb cell 11 for every bit: endpoint counts
//                            into a [K,N] table in one pass, point masks, the kept pairs of every proposal in pair order
// C ABI: include/cppf.h.  Each bit is held to cppf_backvote_ws / cppf_segment_instance bit for bit (tests/test_gpu_scene_multi.py).
//
// The arithmetic that decides a bit is backvote_body's (pose_tail.hip): both kernels call backvote_common.h, where it is derived.
#include "backvote_common.h"
#include "compact.h"

#define BVM_MAX_CENTERS 32
#define BVM_K_BITS 5
#define BVM_MAX_PAIRS ((int64_t)1 << (32 - BVM_K_BITS))   // a queue entry is pair << 5 | k in one word

// ----------------------------------------------------------------------------- back-vote at K centres
__global__ __launch_bounds__(256) void backvote_multi_kernel(const float* __restrict__ points, const float* __restrict__ outputs,
                                                             const int32_t* __restrict__ point_idxs, const float* __restrict__ corner,
                                                             float res, int64_t n_ppfs, int n_rots, int gx, int gy, int gz,
                                                             const float* __restrict__ centers, int n_centers, float tol,
                                                             uint32_t* __restrict__ surv_bits,
                                                             const unsigned long long* __restrict__ vote_ws)
{
    // LDS: (cos, sin) table of every n <= n_rots (when it fits) | per-wave queues, 4 x 128 words | the centres, 3 x n_centers floats
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float2* ltab = reinterpret_cast<float2*>(lds);
    const int entries = n_rots * (n_rots + 1) / 2;
    const bool in_lds = entries <= VOTE_TAB_LDS_MAX;
    float* base_f = lds + (in_lds ? 2 * entries : 0);
    uint32_t* q = reinterpret_cast<uint32_t*>(base_f) + (threadIdx.x >> 6) * 128;
    float* lc = base_f + 4 * 128;
    if (in_lds) bv_load_rot_table(ltab, entries, n_rots, vote_ws);
    for (int e = threadIdx.x; e < 3 * n_centers; e += blockDim.x) lc[e] = centers[e];
    __syncthreads();
    const f3 cr = {corner[0], corner[1], corner[2]};
    const float bx = (float)(gx - 1), by = (float)(gy - 1), bz = (float)(gz - 1);
    const float rinv_res = 1.0f / res;
    const int lane = threadIdx.x & 63;
    int qn = 0;

    // Stage 2, one queued (pair, centre) per lane: the reference's loop over the arc of rotations that can pass :101, in index
    // order, the first passing one wins (backvote_body's `rotations`, with the centre read from LDS per lane).
    auto rotations = [&](const uint32_t item) {
        const int64_t idx = (int64_t)(item >> BVM_K_BITS);
        const int k = (int)(item & (BVM_MAX_CENTERS - 1));
        const f3 gt = {lc[3 * k], lc[3 * k + 1], lc[3 * k + 2]};
        const float2 o = reinterpret_cast<const float2*>(outputs)[idx];
        const int2 ij = reinterpret_cast<const int2*>(point_idxs)[idx];
        f3 a, ab, xd;
        pair_frame(points, ij.x, ij.y, a, ab, xd);
        const float proj_len = o.x, odist = o.y;
        const f3 cc = sub3(a, scl3(ab, proj_len));
        const f3 x = scl3(xd, odist);
        const f3 y = cross3(x, ab);
        const int n = bv_rot_count(odist, res, n_rots);
        const int tbase = n * (n - 1) / 2;
        const f3 dd = sub3(a, ld3(points, ij.y));
        const int2 arc = bv_arc(dot3(dd, dd), sub3(gt, cc), x, y, tol, n, bv_cmax(cc));
        const int lo = arc.x, cnt = arc.y;
        const int p1 = max(0, lo + cnt - n);     // candidates that wrap past n - 1 come first in index order
        for (int kk = 0; kk < cnt; ++kk) {
            const int i = kk < p1 ? kk : lo + (kk - p1);
            const float2 cs = in_lds ? ltab[tbase + i] : rot_cs(i, n);
            const f3 offset = add3(scl3(x, cs.x), scl3(y, cs.y));
            const f3 pc = add3(cc, offset);
            bool done = false, nz = false;         // (flags, not `continue`: the shape that keeps this kernel's registers)
            if (!bv_too_far(pc, gt, tol) && !bv_outside(pc, cr, res, bx, by, bz)) {     // :101, :103-107
                const f3 found = neg3(offset);                                          // :108; a survivor has found != 0
                done = true;
                nz = (found.x != 0.f) || (found.y != 0.f) || (found.z != 0.f);
            }
            if (nz) atomicOr(surv_bits + idx, 1u << k);       // (zeroed by the host entry; integer OR: the same word on every run)
            if (done) break;
        }
    };

    constexpr int BV_U = 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * BV_U;
    for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63)) * BV_U;; base += stride) {
        const bool more = base < n_ppfs;   // wave-uniform
        if (more) {
            float2 o_[BV_U];
            int2 ij_[BV_U];
            f3 pa_[BV_U], pb_[BV_U];
#pragma unroll
            for (int u = 0; u < BV_U; ++u) {
                const int64_t i = base + u * 64 + lane;
                const int64_t c = i < n_ppfs ? i : n_ppfs - 1;
                o_[u] = reinterpret_cast<const float2*>(outputs)[c];
                ij_[u] = reinterpret_cast<const int2*>(point_idxs)[c];
            }
#pragma unroll
            for (int u = 0; u < BV_U; ++u) { pa_[u] = ld3(points, ij_[u].x); pb_[u] = ld3(points, ij_[u].y); }
#pragma unroll
            for (int u = 0; u < BV_U; ++u) {
                const int64_t idx = base + u * 64 + lane;
                // the pair's part of stage 1, once: mode 0 = no centre can pass, 1 = the approximate circle test, 2 = (nearly)
                // coincident points, where the exact frame decides what is degenerate and every centre goes on to stage 2.
                // (backvote_body's two screens, derived there, split into this part and the centre's below: a change to a formula
                // or a bound belongs in both.)
                int mode = 0;
                f3 cc = {0.f, 0.f, 0.f}, ax = {0.f, 0.f, 0.f};
                float rho = 0.f, squash = 0.f;
                if (idx < n_ppfs) {
                    const float2 o = o_[u];
                    const f3 pa = pa_[u], pb = pb_[u];
                    const f3 dd = sub3(pa, pb);
                    const float L2 = dot3(dd, dd);
                    if (L2 >= 1e-13f) {
                        const float L = __builtin_amdgcn_sqrtf(L2);
                        const float inv = __builtin_amdgcn_rcpf(L + 1e-7f);
                        const float proj_len = o.x, odist = o.y;
                        ax = scl3(dd, inv);
                        cc = sub3(pa, scl3(ax, proj_len));
                        rho = fabsf(odist);
                        squash = (rho + fabsf(proj_len)) * 2e-7f * inv;
                        mode = (odist * rinv_res * 6.2831855f >= 0.9999f) ? 1 : 0;
                    } else {
                        const int2 ij = ij_[u];
                        f3 a, ab, xd;
                        if (pair_frame(points, ij.x, ij.y, a, ab, xd)) mode = bv_rot_count(o.y, res, n_rots) > 0 ? 2 : 0;
                    }
                }
                if (__any(mode != 0)) {
                    for (int k = 0; k < n_centers; ++k) {      // wave-uniform: the centre is a broadcast read
                        const f3 gt = {lc[3 * k], lc[3 * k + 1], lc[3 * k + 2]};
                        bool pass = false;
                        if (mode == 1) {
                            // distance from the centre to the vote circle (centre cc, axis ax, radius |nu|): backvote_body, stage 1
                            const f3 w = sub3(gt, cc);
                            const float h = dot3(w, ax), w2 = dot3(w, w);
                            const float r = __builtin_amdgcn_sqrtf(fmaxf(w2 - h * h, 0.f));
                            const float dist = __builtin_amdgcn_sqrtf((r - rho) * (r - rho) + h * h);
                            const float mag = __builtin_amdgcn_sqrtf(w2) + rho + tol;
                            pass = !(dist > tol + 2e-4f * mag + 1e-6f + squash);
                        } else if (mode == 2) {
                            pass = true;       // no screen for these: their samples lie on an ellipse (backvote_body, stage 1)
                        }
                        if (!__any(pass)) continue;
                        qn += bv_push(q + qn, pass, ((uint32_t)idx << BVM_K_BITS) | (uint32_t)k);
                        if (qn >= 64) {                        // (qn < 64 before the push and <= 64 pushed: one drain, < 128 entries)
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                            const uint32_t item = q[qn - 64 + lane];
                            qn -= 64;
                            rotations(item);
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        }
                    }
                }
            }
        }
        if (!more) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (lane < qn) rotations(q[lane]);
            break;
        }
    }
}

extern "C" int cppf_backvote_multi(const float* points, const float* outputs, const int32_t* point_idxs, const float* corner, float res,
                                   int64_t n_ppfs, int n_rots, int gx, int gy, int gz, const float* centers, int n_centers, float tol,
                                   uint32_t* surv_bits, const void* vote_workspace, void* stream)
{
    if (n_centers < 1 || n_centers > BVM_MAX_CENTERS || n_rots < 1 || n_rots > CPPF_MAX_ROTS || n_ppfs < 0 || n_ppfs >= BVM_MAX_PAIRS)
        return CPPF_EINVAL;
    if (gx < 1 || gy < 1 || gz < 1) return CPPF_EINVAL;
    if (n_ppfs == 0) return 0;
    if (!points || !outputs || !point_idxs || !corner || !centers || !surv_bits) return CPPF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(surv_bits, 0, (size_t)n_ppfs * sizeof(uint32_t), st)) return (int)e;
    const size_t lds = backvote_lds_bytes(n_rots, 3 * BVM_MAX_CENTERS * sizeof(float));
    hipLaunchKernelGGL(backvote_multi_kernel, dim3((unsigned)backvote_blocks(n_ppfs)), dim3(256), lds, st, points, outputs, point_idxs,
                       corner, res, n_ppfs, n_rots, gx, gy, gz, centers, n_centers, tol, surv_bits, static_cast<const unsigned long long*>(vote_workspace));
    CPPF_CHECK_LAUNCH();
    return 0;
}

// ----------------------------------------------------------------------------- segmentation of all proposals
// contrib[k][n] = how often point n is an endpoint of a survivor of proposal k: one pass over the pair list for every k (integer
// atomics: the same counts on every run; a pair (i, i) counts twice, as in endpoint_hist_kernel of scene.hip)
__global__ __launch_bounds__(256) void endpoint_hist_multi_kernel(const int32_t* __restrict__ idx, const uint32_t* __restrict__ surv_bits,
                                                                  int64_t n_pairs, int64_t n_points, uint32_t k_mask,
                                                                  int32_t* __restrict__ contrib)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        uint32_t bits = surv_bits[p] & k_mask;
        if (!bits) continue;
        const int2 ij = reinterpret_cast<const int2*>(idx)[p];
        const bool a = ij.x >= 0 && ij.x < n_points, b = ij.y >= 0 && ij.y < n_points;
        while (bits) {
            const int k = __builtin_ctz(bits);
            bits &= bits - 1;
            if (a) atomicAdd(contrib + (int64_t)k * n_points + ij.x, 1);
            if (b) atomicAdd(contrib + (int64_t)k * n_points + ij.y, 1);
        }
    }
}

__global__ __launch_bounds__(256) void point_masks_kernel(const int32_t* __restrict__ contrib, int64_t n, int min_contrib,
                                                          uint8_t* __restrict__ point_masks)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        point_masks[i] = contrib[i] > min_contrib ? 1 : 0;
}

// keep_bits[p] bit k = pair p survives at proposal k and has an endpoint in its point mask; counts[k][chunk] = the kept pairs of
// proposal k among the chunk's CMP_BLOCK pairs.  One block per chunk.
__global__ __launch_bounds__(CMP_BLOCK) void keep_count_multi_kernel(const int32_t* __restrict__ idx, const uint32_t* __restrict__ surv_bits,
                                                                     int64_t n_pairs, int64_t n_points, int n_centers, uint32_t k_mask,
                                                                     const uint8_t* __restrict__ point_masks,
                                                                     uint32_t* __restrict__ keep_bits, int32_t* __restrict__ counts,
                                                                     int64_t n_chunks)
{
    __shared__ int wsum[CMP_BLOCK / 64][BVM_MAX_CENTERS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x;
    uint32_t keep = 0;
    if (p < n_pairs) {
        uint32_t bits = surv_bits[p] & k_mask;
        if (bits) {
            const int2 ij = reinterpret_cast<const int2*>(idx)[p];
            const bool a = ij.x >= 0 && ij.x < n_points, b = ij.y >= 0 && ij.y < n_points;
            while (bits) {
                const int k = __builtin_ctz(bits);
                bits &= bits - 1;
                const uint8_t* pm = point_masks + (int64_t)k * n_points;
                if ((a && pm[ij.x]) || (b && pm[ij.y])) keep |= 1u << k;
            }
        }
        keep_bits[p] = keep;
    }
    int mine = 0;
    for (int k = 0; k < n_centers; ++k) {
        const int c = __popcll(__ballot((keep >> k) & 1u));
        if (lane == k) mine = c;
    }
    if (lane < n_centers) wsum[w][lane] = mine;
    __syncthreads();
    if ((int)threadIdx.x < n_centers) {
        int s = 0;
        for (int k = 0; k < CMP_BLOCK / 64; ++k) s += wsum[k][threadIdx.x];
        counts[(int64_t)threadIdx.x * n_chunks + blockIdx.x] = s;
    }
}

// exclusive scan in place over the flat [n_centers][n_chunks] table (proposal-major: the lists follow each other), and
// offsets[k] = the scan at the start of row k, offsets[n_centers] = the total.  One block, 1024 entries per sweep.
__global__ __launch_bounds__(1024) void scan_multi_kernel(int32_t* __restrict__ counts, int64_t n_chunks, int n_centers,
                                                          int32_t* __restrict__ offsets)
{
    __shared__ int wtot[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t n = n_chunks * n_centers;
    if (n == 0) {
        if ((int)threadIdx.x <= n_centers) offsets[threadIdx.x] = 0;
        return;
    }
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        int before = carry_s;
        for (int k = 0; k < w; ++k) before += wtot[k];
        const int excl = before + incl - v;
        if (i < n) {
            counts[i] = excl;
            if (i % n_chunks == 0) offsets[i / n_chunks] = excl;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = excl + v;
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[n_centers] = carry_s;
}

// pairs_out[starts[k][chunk] + rank within the chunk] = p for every kept (p, k), positions >= capacity dropped
__global__ __launch_bounds__(CMP_BLOCK) void scatter_multi_kernel(const uint32_t* __restrict__ keep_bits, int64_t n_pairs, int n_centers,
                                                                  const int32_t* __restrict__ starts, int64_t n_chunks,
                                                                  int32_t* __restrict__ pairs_out, int64_t capacity)
{
    __shared__ int wsum[CMP_BLOCK / 64][BVM_MAX_CENTERS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * CMP_BLOCK + threadIdx.x;
    const uint32_t keep = p < n_pairs ? keep_bits[p] : 0u;
    int mine = 0;
    for (int k = 0; k < n_centers; ++k) {
        const int c = __popcll(__ballot((keep >> k) & 1u));
        if (lane == k) mine = c;
    }
    if (lane < n_centers) wsum[w][lane] = mine;
    __syncthreads();
    for (int k = 0; k < n_centers; ++k) {
        const bool f = (keep >> k) & 1u;
        const unsigned long long b = __ballot(f);
        if (b == 0ull) continue;
        int woff = 0;
        for (int j = 0; j < w; ++j) woff += wsum[j][k];
        if (f) {
            const int64_t pos = (int64_t)starts[(int64_t)k * n_chunks + blockIdx.x] + woff + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < capacity) pairs_out[pos] = (int32_t)p;
        }
    }
}

static int64_t chunks_of(int64_t n_pairs) { return (n_pairs + CMP_BLOCK - 1) / CMP_BLOCK; }

extern "C" size_t cppf_segment_instances_workspace_bytes(int64_t n_points, int64_t n_pairs, int n_centers)
{
    if (n_points < 0 || n_pairs < 0 || n_centers < 1 || n_centers > BVM_MAX_CENTERS) return 0;
    return align256((size_t)n_centers * n_points * sizeof(int32_t)) + align256((size_t)n_pairs * sizeof(uint32_t)) +
           align256((size_t)(chunks_of(n_pairs) * n_centers + 1) * sizeof(int32_t));
}

extern "C" int cppf_segment_instances(const int32_t* point_idxs, const uint32_t* surv_bits, int64_t n_pairs, int64_t n_points,
                                      int n_centers, int min_contrib, uint8_t* point_masks, int32_t* pairs_out, int64_t capacity,
                                      int32_t* offsets, void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_centers < 1 || n_centers > BVM_MAX_CENTERS || n_pairs < 0 || n_points < 1 || n_points > INT32_MAX || capacity < 0)
        return CPPF_EINVAL;
    if (!point_masks || !offsets || (capacity > 0 && !pairs_out) || (n_pairs > 0 && (!point_idxs || !surv_bits))) return CPPF_EINVAL;
    if (n_pairs * n_centers > INT32_MAX) return CPPF_EUNSUPPORTED;                   // offsets are int32
    if (!workspace || workspace_bytes < cppf_segment_instances_workspace_bytes(n_points, n_pairs, n_centers)) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nc = chunks_of(n_pairs);
    const size_t cb = align256((size_t)n_centers * n_points * sizeof(int32_t)), kb = align256((size_t)n_pairs * sizeof(uint32_t));
    int32_t* contrib = static_cast<int32_t*>(workspace);
    uint32_t* keep_bits = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + cb);
    int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + cb + kb);
    const uint32_t k_mask = n_centers == 32 ? 0xffffffffu : ((1u << n_centers) - 1u);
    if (hipError_t e = hipMemsetAsync(contrib, 0, (size_t)n_centers * n_points * sizeof(int32_t), st)) return (int)e;
    if (n_pairs > 0)
        hipLaunchKernelGGL(endpoint_hist_multi_kernel, dim3(blocks256(n_pairs)), dim3(256), 0, st, point_idxs, surv_bits, n_pairs,
                           n_points, k_mask, contrib);
    hipLaunchKernelGGL(point_masks_kernel, dim3(blocks256((int64_t)n_centers * n_points)), dim3(256), 0, st, contrib,
                       (int64_t)n_centers * n_points, min_contrib, point_masks);
    if (n_pairs > 0)
        hipLaunchKernelGGL(keep_count_multi_kernel, dim3((unsigned)nc), dim3(CMP_BLOCK), 0, st, point_idxs, surv_bits, n_pairs, n_points,
                           n_centers, k_mask, point_masks, keep_bits, counts, nc);
    hipLaunchKernelGGL(scan_multi_kernel, dim3(1), dim3(1024), 0, st, counts, nc, n_centers, offsets);
    if (n_pairs > 0 && capacity > 0)
        hipLaunchKernelGGL(scatter_multi_kernel, dim3((unsigned)nc), dim3(CMP_BLOCK), 0, st, keep_bits, n_pairs, n_centers, counts, nc,
                           pairs_out, capacity);
    CPPF_CHECK_LAUNCH();
    return 0;
}
