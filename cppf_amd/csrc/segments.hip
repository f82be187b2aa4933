// Segments of a depth frame for gfx950 (MI355X): connected components of the depth image under a depth-discontinuity rule, and a
// RANSAC plane fit to cut the support surface away first.  C ABI and the definitions: include/cppf.h ("Depth segments"); host side:
// cppf_amd/segments.py; restated in numpy / scipy: tests/segments_ref.py.
//
// cppf_depth_segments, seven launches over two caller arrays A = labels and B = comp_size:
//   seg_init_kernel     A[p] = the start of p's run of left-linked pixels inside its wave's 64 flat indices (one ballot), -1 for a
//                       dead pixel; B[p] = 0; counts = 0
//   seg_merge_kernel    union-find over A with the smaller index as the parent: a pixel joins its upper neighbour (skipped where the
//                       link is implied by the pixel to its left), lane 0 of a wave joins the run to its left.  Workgroups lower each
//                       other's parents here, so EVERY access to A in this kernel is an agent-scope atomic: relaxed atomic loads to
//                       follow parents, atomic min to lower one (per-XCD L2s are not coherent for plain accesses).
//   seg_count_kernel    A is read-only (after a kernel boundary): root = find(p); a non-root keeps root + 1 in its OWN B[p]; the
//                       component size is counted DOWN in B[root] with one atomic add per distinct root of a wave -- B[root] is
//                       touched by atomics alone in this kernel
//   seg_collect_kernel  the roots (A[p] == p) whose size passes the filter take slots of `first` by ballot + one counter; counts
//   seg_rank_kernel     one workgroup: the kept roots ranked in LDS (a rank is a count of smaller roots: no ticket order survives),
//                       first / sizes written in rank order, the tail of both defined
//   seg_label_kernel    NON-roots: size from B[root] (roots do not write in this kernel), rank by binary search of `first` in LDS
//   seg_roots_kernel    roots: their own two entries
// Every cross-workgroup hand-over besides seg_merge_kernel's is a kernel boundary.  Integer atomics only: the same bits on every run.
//
// cppf_plane_ransac: pr_planes_kernel (one lane per hypothesis: Philox stream 5, three points, the plane in fp32), pr_count_kernel
// (planes staged in LDS and read as broadcasts; a wave counts a plane's inliers with one ballot, lane 0 adds to the workgroup's LDS
// counter; one global integer add per plane and workgroup), pr_best_kernel (one workgroup: arg-max, lowest index on ties).
// No allocation, no host synchronisation, vector stores only: both calls can be captured in a graph.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"
#include "cppf_math.h"

#define SEG_BLOCK 256
#define SEG_MAX CPPF_SEGMENTS_MAX
#define SEG_MAX_PIXELS (1 << 24)
#define PR_BLOCK 256
#define PR_MAX_HYP CPPF_PLANE_MAX_HYPOTHESES
#define PR_MAX_BLOCKS 512
#define PR_STREAM 5u                     // Philox counter word 2; 0..4 are taken (cppf_math.h, scene_train.hip)

// ------------------------------------------------------------------------------------------------ depth segments
__device__ __forceinline__ int seg_depth(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ valid, int p)
{
    const int z = depth[p];
    return (z > 0 && (!valid || valid[p])) ? z : 0;
}

__device__ __forceinline__ bool seg_linked(int za, int zb, int tol, int slope)
{
    if (za <= 0 || zb <= 0) return false;
    const int lo = za < zb ? za : zb, hi = za < zb ? zb : za;
    return hi - lo <= tol + (slope * lo) / 1000;                               // slope <= 1000, lo <= 65535: no overflow
}

__device__ __forceinline__ int seg_load(const int32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int seg_find_atomic(const int32_t* A, int x)
{
    for (int y = seg_load(A + x); y != x; y = seg_load(A + x)) x = y;
    return x;
}

__device__ __forceinline__ void seg_union(int32_t* A, int a, int b)
{
    bool done;
    do {
        a = seg_find_atomic(A, a);
        b = seg_find_atomic(A, b);
        if (a < b) {
            const int old = __hip_atomic_fetch_min(A + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = __hip_atomic_fetch_min(A + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_init_kernel(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ valid, int W, int n,
                                                             int tol, int slope, int32_t* __restrict__ A, int32_t* __restrict__ B,
                                                             int32_t* __restrict__ counts)
{
    const int p = blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (p < 4) counts[p] = 0;                                                  // (n >= 1 and a block is 256 wide: block 0 has them)
    const bool in = p < n;
    const int z = in ? seg_depth(depth, valid, p) : 0;
    const bool left = in && z > 0 && (p % W) != 0 && seg_linked(z, seg_depth(depth, valid, p - 1), tol, slope);
    // the run of left-linked pixels p belongs to, inside this wave's 64 consecutive flat indices: its first pixel is the parent
    const unsigned long long linked = __ballot(left);
    const int lane = threadIdx.x & 63;
    // lanes <= mine that start a run; lane 0 always does (seg_merge_kernel joins it to the wave before)
    const unsigned long long breaks = (~linked | 1ull) & ((2ull << lane) - 1);
    const int start = 63 - __clzll((long long)breaks);
    if (!in) return;
    B[p] = 0;
    A[p] = z > 0 ? p - (lane - start) : -1;
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_merge_kernel(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ valid, int W, int n,
                                                              int tol, int slope, int32_t* A)
{
    const int p = blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int z = seg_depth(depth, valid, p);
    if (z <= 0) return;
    const int x = p % W;
    const int zl = x ? seg_depth(depth, valid, p - 1) : 0;
    const bool left = seg_linked(z, zl, tol, slope);
    if (left && (threadIdx.x & 63) == 0) seg_union(A, p, p - 1);               // the run continues in the wave before this one
    if (p >= W) {
        const int zu = seg_depth(depth, valid, p - W);
        if (seg_linked(z, zu, tol, slope)) {
            // p ~ p-1 ~ p-1-W ~ p-W already: the pixel to the left makes this join
            const bool implied = left && seg_linked(zl, seg_depth(depth, valid, p - 1 - W), tol, slope)
                                 && seg_linked(zu, seg_depth(depth, valid, p - 1 - W), tol, slope);
            if (!implied) seg_union(A, p, p - W);
        }
    }
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_count_kernel(const int32_t* __restrict__ A, int n, int32_t* B)
{
    const int p = blockIdx.x * SEG_BLOCK + threadIdx.x;
    int r = -1;
    if (p < n && A[p] >= 0) {
        r = p;
        for (int y = A[r]; y != r; y = A[r]) r = y;
        if (r != p) B[p] = r + 1;                                              // my own word: nobody counts into a non-root
    }
    // one atomic per distinct root of the wave
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int rl = __shfl(r, leader, 64);
        const unsigned long long same = __ballot(r == rl);
        if (lane == leader) atomicAdd(B + rl, -__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ bool seg_kept(int size, int min_pixels, int max_pixels)
{
    return size >= min_pixels && (max_pixels == 0 || size <= max_pixels);
}

__global__ __launch_bounds__(SEG_BLOCK) void seg_collect_kernel(const int32_t* __restrict__ A, const int32_t* __restrict__ B, int n, int min_pixels,
                                                                int max_pixels, int capacity, int32_t* __restrict__ first, int32_t* counts)
{
    const int p = blockIdx.x * SEG_BLOCK + threadIdx.x;
    const bool live = p < n && A[p] >= 0;
    const bool root = live && A[p] == p;
    const bool kept = root && seg_kept(-B[p], min_pixels, max_pixels);
    const unsigned long long m_live = __ballot(live), m_root = __ballot(root), m_kept = __ballot(kept);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) {
        if (m_live) atomicAdd(counts + 2, __popcll(m_live));
        if (m_root) atomicAdd(counts + 1, __popcll(m_root));
        if (m_kept) base = atomicAdd(counts + 0, __popcll(m_kept));
    }
    base = __shfl(base, 0, 64);
    if (kept) {
        const int slot = base + __popcll(m_kept & ((1ull << lane) - 1));
        if (slot < capacity) first[slot] = p;                                  // ticket order: seg_rank_kernel sorts it away
    }
}

__global__ __launch_bounds__(SEG_MAX) void seg_rank_kernel(const int32_t* __restrict__ B, const int32_t* __restrict__ counts, int capacity,
                                                           int32_t* __restrict__ first, int32_t* __restrict__ sizes)
{
    __shared__ int s_root[SEG_MAX];
    const int t = threadIdx.x;
    const int S = counts[0];
    const int m = S <= capacity ? S : 0;                                       // overflow: nothing is listed (and nothing labelled)
    const int mine = t < m ? first[t] : 0x7fffffff;
    s_root[t] = mine;
    __syncthreads();
    int rank = 0;
    if (t < m)
        for (int j = 0; j < m; ++j) rank += s_root[j] < mine;                  // roots are distinct: the ranks are a permutation
    __syncthreads();                                                           // (every read of first[] above is done)
    if (t < m) {
        first[rank] = mine;
        sizes[rank] = -B[mine];
    } else if (t < capacity) {
        first[t] = -1;
        sizes[t] = 0;
    }
}

__device__ __forceinline__ int seg_rank_of(const int* s_first, int m, int r)
{
    int lo = 0, hi = m;                                                        // the first entry >= r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_first[mid] < r) lo = mid + 1; else hi = mid;
    }
    return (lo < m && s_first[lo] == r) ? lo : -1;
}

// roots == 0: every live pixel that is not a root; roots == 1: the roots.  A[p] == p still marks a root after the first of the two: a
// non-root's rank is below its root's index, which is below p.
template <int ROOTS>
__global__ __launch_bounds__(SEG_BLOCK) void seg_label_kernel(int32_t* A, int32_t* B, int n, const int32_t* __restrict__ first,
                                                              const int32_t* __restrict__ counts, int capacity)
{
    __shared__ int s_first[SEG_MAX];
    const int S = counts[0];
    const int m = S <= capacity ? S : 0;
    for (int t = threadIdx.x; t < m; t += SEG_BLOCK) s_first[t] = first[t];
    __syncthreads();
    const int p = blockIdx.x * SEG_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int a = A[p];
    if (a < 0 || (a == p) != (ROOTS == 1)) return;                             // dead pixels are final since seg_init_kernel: {-1, 0}
    const int r = ROOTS ? p : B[p] - 1;
    B[p] = -B[r];
    A[p] = seg_rank_of(s_first, m, r);
}

extern "C" int cppf_depth_segments(const int16_t* depth, const uint8_t* valid, int H, int W, int tol_mm, int slope_permille, int min_pixels,
                                   int max_pixels, int capacity, int32_t* labels, int32_t* comp_size, int32_t* first, int32_t* sizes,
                                   int32_t* counts, void* stream)
{
    if (H < 1 || W < 1 || (int64_t)H * W > SEG_MAX_PIXELS) return CPPF_EINVAL;
    if (tol_mm < 0 || tol_mm > 65535 || slope_permille < 0 || slope_permille > 1000) return CPPF_EINVAL;
    if (min_pixels < 1 || max_pixels < 0 || capacity < 1 || capacity > SEG_MAX) return CPPF_EINVAL;
    if (!depth || !labels || !comp_size || !first || !sizes || !counts) return CPPF_EINVAL;
    const int n = H * W;
    const dim3 grid((unsigned)((n + SEG_BLOCK - 1) / SEG_BLOCK)), block(SEG_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    const uint16_t* d = (const uint16_t*)depth;
    hipLaunchKernelGGL(seg_init_kernel, grid, block, 0, s, d, valid, W, n, tol_mm, slope_permille, labels, comp_size, counts);
    hipLaunchKernelGGL(seg_merge_kernel, grid, block, 0, s, d, valid, W, n, tol_mm, slope_permille, labels);
    hipLaunchKernelGGL(seg_count_kernel, grid, block, 0, s, labels, n, comp_size);
    hipLaunchKernelGGL(seg_collect_kernel, grid, block, 0, s, labels, comp_size, n, min_pixels, max_pixels, capacity, first, counts);
    hipLaunchKernelGGL(seg_rank_kernel, dim3(1), dim3(SEG_MAX), 0, s, comp_size, counts, capacity, first, sizes);
    hipLaunchKernelGGL(seg_label_kernel<0>, grid, block, 0, s, labels, comp_size, n, first, counts, capacity);
    hipLaunchKernelGGL(seg_label_kernel<1>, grid, block, 0, s, labels, comp_size, n, first, counts, capacity);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}

// ------------------------------------------------------------------------------------------------ plane RANSAC
__global__ __launch_bounds__(PR_BLOCK) void pr_planes_kernel(const float* __restrict__ points, uint32_t n_points, int n_hyp, uint2 key,
                                                             float4* __restrict__ planes, int32_t* __restrict__ counts)
{
    const int h = blockIdx.x * PR_BLOCK + threadIdx.x;
    if (h >= n_hyp) return;
    using namespace cppf;
    const uint4 w = philox4x32_10(make_uint4((unsigned)h, 0u, PR_STREAM, 0u), key);
    const int64_t ia = (int64_t)(((unsigned long long)w.x * n_points) >> 32), ib = (int64_t)(((unsigned long long)w.y * n_points) >> 32),
                  ic = (int64_t)(((unsigned long long)w.z * n_points) >> 32);
    const f3 a = {points[3 * ia], points[3 * ia + 1], points[3 * ia + 2]}, b = {points[3 * ib], points[3 * ib + 1], points[3 * ib + 2]},
             c = {points[3 * ic], points[3 * ic + 1], points[3 * ic + 2]};
    const f3 e1 = sub3(b, a), e2 = sub3(c, a);
    f3 nn = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
    const float l = sqrtf((nn.x * nn.x + nn.y * nn.y) + nn.z * nn.z);
    const bool finite9 = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(c.x) &&
                         isfinite(c.y) && isfinite(c.z);
    float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (finite9 && l > 1e-12f) {
        nn = div3(nn, l);
        float d = -((nn.x * a.x + nn.y * a.y) + nn.z * a.z);
        if (d < 0.f) { nn = neg3(nn); d = -d; }
        // a normal whose three components all underflowed, or a plane that is not finite, would pass for "degenerate" / count garbage
        if (isfinite(d) && isfinite(nn.x) && isfinite(nn.y) && isfinite(nn.z) && (nn.x != 0.f || nn.y != 0.f || nn.z != 0.f))
            pl = make_float4(nn.x, nn.y, nn.z, d);
    }
    planes[h] = pl;
    counts[h] = 0;
}

__global__ __launch_bounds__(PR_BLOCK) void pr_count_kernel(const float* __restrict__ points, int64_t n_points, int n_hyp, float thresh,
                                                            const float4* __restrict__ planes, int32_t* counts)
{
    __shared__ float4 s_pl[PR_MAX_HYP];
    __shared__ int s_cnt[PR_MAX_HYP];
    for (int h = threadIdx.x; h < n_hyp; h += PR_BLOCK) {
        s_pl[h] = planes[h];
        s_cnt[h] = 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * PR_BLOCK;
    // every lane of a wave makes the same number of trips (the ballots need the whole wave): the bound is the wave's first index
    for (int64_t base = (int64_t)blockIdx.x * PR_BLOCK + (threadIdx.x & ~63); base < n_points; base += stride) {
        const int64_t i = base + lane;
        const bool in = i < n_points;
        float x = 0.f, y = 0.f, z = 0.f;
        if (in) { x = points[3 * i]; y = points[3 * i + 1]; z = points[3 * i + 2]; }
        for (int h = 0; h < n_hyp; ++h) {
            const float4 pl = s_pl[h];                                         // one address for the wave: a broadcast
            if (pl.x == 0.f && pl.y == 0.f && pl.z == 0.f) continue;           // degenerate (uniform over the wave)
            const bool hit = in && fabsf(((pl.x * x + pl.y * y) + pl.z * z) + pl.w) <= thresh;      // NaN / inf compare false
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(s_cnt + h, __popcll(m));
        }
    }
    __syncthreads();
    for (int h = threadIdx.x; h < n_hyp; h += PR_BLOCK)
        if (s_cnt[h]) atomicAdd(counts + h, s_cnt[h]);
}

__global__ __launch_bounds__(PR_MAX_HYP) void pr_best_kernel(const float4* __restrict__ planes, const int32_t* __restrict__ counts, int n_hyp,
                                                             int32_t* __restrict__ best)
{
    // key = count << 10 | (1023 - h) over the non-degenerate hypotheses: the largest key is the largest count at the lowest h
    __shared__ long long s_key[PR_MAX_HYP];
    const int t = threadIdx.x;
    long long key = -1;
    if (t < n_hyp) {
        const float4 pl = planes[t];
        if (pl.x != 0.f || pl.y != 0.f || pl.z != 0.f) key = ((long long)counts[t] << 10) | (long long)(PR_MAX_HYP - 1 - t);
    }
    s_key[t] = key;
    __syncthreads();
    for (int w = PR_MAX_HYP / 2; w > 0; w >>= 1) {
        if (t < w && s_key[t + w] > s_key[t]) s_key[t] = s_key[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const long long k = s_key[0];
        best[0] = k < 0 ? -1 : PR_MAX_HYP - 1 - (int)(k & (PR_MAX_HYP - 1));
        best[1] = k < 0 ? 0 : (int)(k >> 10);
    }
}

extern "C" int cppf_plane_ransac(const float* points, int64_t n_points, int n_hyp, float thresh, unsigned long long seed, float* planes,
                                 int32_t* counts, int32_t* best, void* stream)
{
    if (n_points < 1 || n_points > INT32_MAX || n_hyp < 1 || n_hyp > PR_MAX_HYP) return CPPF_EINVAL;
    if (!(thresh >= 0.f) || !isfinite(thresh)) return CPPF_EINVAL;
    if (!points || !planes || !counts || !best) return CPPF_EINVAL;
    if ((uintptr_t)planes & 15u) return CPPF_EINVAL;                           // a plane is stored as one 16-byte word
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pr_planes_kernel, dim3((unsigned)((n_hyp + PR_BLOCK - 1) / PR_BLOCK)), dim3(PR_BLOCK), 0, s, points, (uint32_t)n_points,
                       n_hyp, make_uint2((unsigned)seed, (unsigned)(seed >> 32)), (float4*)planes, counts);
    int64_t blocks = (n_points + PR_BLOCK - 1) / PR_BLOCK;
    if (blocks > PR_MAX_BLOCKS) blocks = PR_MAX_BLOCKS;
    hipLaunchKernelGGL(pr_count_kernel, dim3((unsigned)blocks), dim3(PR_BLOCK), 0, s, points, n_points, n_hyp, thresh, (const float4*)planes, counts);
    hipLaunchKernelGGL(pr_best_kernel, dim3(1), dim3(PR_MAX_HYP), 0, s, (const float4*)planes, counts, n_hyp, best);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}
