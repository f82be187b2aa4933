// The zero-shot scene path of nocs/zero_shot.ipynb for gfx950 (MI355X): what turns one whole-scene vote grid into objects.
//   cell 6   pair filter ("indistinguishable" pairs)         cppf_pair_filter_distinct
//   cell 9   Gaussian smoothing of the grid                  cppf_gaussian_filter3d
//            iterative peak proposals                        cppf_scene_proposals (one workgroup runs the whole loop)
//   cell 11  unsupervised instance segmentation            cppf_segment_instance
// C ABI and the defined behaviour where the notebook has none: include/cppf.h.  The numpy restatement the tests hold these
// kernels to, bit for bit: tests/zero_shot_ref.py.
#include "backvote_common.h"

#define SCN_TILE 8                    // proposals: the max table holds one (value, first index) per 8^3 cells
#define SCN_TILE_CELLS (SCN_TILE * SCN_TILE * SCN_TILE)
#define SCN_LOOP_THREADS 1024
#define SCN_MAX_RADIUS 32             // (tested at 0, 31 and 32; 33 is refused -- tests/test_gpu_limits.py)
#define SCN_MAX_MARGIN 64             // an edge slice holds <= 2 * margin <= 128 cells: numpy's pairwise_sum base case (tested at
                                      // 1 and 64 on a 140 x 137 x 131 grid -- tests/test_gpu_limits.py)

struct GaussWeights { double w[2 * SCN_MAX_RADIUS + 1]; };
struct TileMax { float v; int32_t i; };

// ----------------------------------------------------------------------------- Gaussian smoothing (cell 9, line 1)
// scipy.ndimage.gaussian_filter(grid, sigma, mode='reflect'): one correlate1d per axis, axes 0, 1, 2.  scipy converts each line
// to fp64, extends it ('reflect' = d c b a | a b c d | d c b a, repeated for lines shorter than the radius) and, for symmetric
// weights, forms w[r] x[c] + sum_{d = r..1} (x[c-d] + x[c+d]) w[r-d] in that order; the pass output is rounded to float32.
__device__ __forceinline__ int reflect_idx(int k, int n)
{
    const int p = 2 * n;
    int m = k % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

__global__ __launch_bounds__(256) void gauss_pass_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         float* __restrict__ out2, int n_cells, int stride, int n_ax,
                                                         int radius, GaussWeights W)
{
    // (grids of < 2^31 cells: 32-bit index arithmetic)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += gridDim.x * blockDim.x) {
        const int c = (i / stride) % n_ax;
        const float* line = in + (i - c * stride);
        double acc = (double)in[i] * W.w[radius];
        for (int d = radius; d > 0; --d) {
            const double a = (double)line[reflect_idx(c - d, n_ax) * stride];
            const double b = (double)line[reflect_idx(c + d, n_ax) * stride];
            acc += (a + b) * W.w[radius - d];
        }
        const float r = (float)acc;
        out[i] = r;
        if (out2) out2[i] = r;
    }
}

static int check_weights(const double* w, int radius, GaussWeights* W)
{
    if (!w || radius < 0 || radius > SCN_MAX_RADIUS) return CPPF_EINVAL;
    for (int k = 0; k <= 2 * radius; ++k) {
        if (w[k] != w[2 * radius - k]) return CPPF_EINVAL;   // scipy's symmetric branch is the one restated
        W->w[k] = w[k];
    }
    return 0;
}

// the three passes: in -> a -> b -> a (+ out2)
static int gauss3(const float* in, float* a, float* b, float* out2, int gx, int gy, int gz, const GaussWeights& W, int radius,
                  hipStream_t st)
{
    const int n = gx * gy * gz;
    const int blocks = (n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192;
    const int strides[3] = {gy * gz, gz, 1};
    const int lens[3] = {gx, gy, gz};
    const float* src[3] = {in, a, b};
    float* dst[3] = {a, b, a};
    for (int ax = 0; ax < 3; ++ax)
        hipLaunchKernelGGL(gauss_pass_kernel, dim3(blocks), dim3(256), 0, st, src[ax], dst[ax], ax == 2 ? out2 : (float*)nullptr, n,
                           strides[ax], lens[ax], radius, W);
    CPPF_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t cppf_gaussian_filter3d_workspace_bytes(int gx, int gy, int gz)
{
    if (gx < 1 || gy < 1 || gz < 1) return 0;
    return align256((size_t)gx * gy * gz * sizeof(float));
}

extern "C" int cppf_gaussian_filter3d(const float* grid, float* out, int gx, int gy, int gz, const double* weights, int radius,
                                      void* workspace, size_t workspace_bytes, void* stream)
{
    if (!grid || !out || grid == out || gx < 1 || gy < 1 || gz < 1) return CPPF_EINVAL;
    if ((int64_t)gx * gy * gz >= ((int64_t)1 << 30)) return CPPF_EUNSUPPORTED;   // 32-bit index arithmetic
    GaussWeights W;
    if (int rc = check_weights(weights, radius, &W)) return rc;
    if (!workspace || workspace_bytes < cppf_gaussian_filter3d_workspace_bytes(gx, gy, gz)) return CPPF_EWORKSPACE;
    // in -> out -> tmp -> out
    return gauss3(grid, out, static_cast<float*>(workspace), nullptr, gx, gy, gz, W, radius, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------- proposals (cell 9, the loop)
// np.argmax order: the larger value, ties to the lower flat index
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// arg-max of (v, i) over the block (blockDim.x a multiple of 64, <= 1024); every thread returns the result
__device__ __forceinline__ void block_argmax(float& v, int& i)
{
    __shared__ float sv[SCN_LOOP_THREADS / 64];
    __shared__ int si[SCN_LOOP_THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (better(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

// (max, first index) of tile (tx, ty, tz); cells beyond the grid are skipped
__device__ __forceinline__ void tile_argmax(const float* __restrict__ g, int gx, int gy, int gz, int tx, int ty, int tz,
                                            float& v, int& i)
{
    v = -INFINITY; i = INT32_MAX;
    for (int t = threadIdx.x; t < SCN_TILE_CELLS; t += blockDim.x) {
        const int x = tx * SCN_TILE + (t >> 6), y = ty * SCN_TILE + ((t >> 3) & 7), z = tz * SCN_TILE + (t & 7);
        if (x < gx && y < gy && z < gz) {
            const int f = (x * gy + y) * gz + z;
            const float c = g[f];
            if (better(c, f, v, i)) { v = c; i = f; }
        }
    }
    block_argmax(v, i);
}

__global__ __launch_bounds__(256) void tile_max_kernel(const float* __restrict__ g, int gx, int gy, int gz, int ntx, int nty, int ntz,
                                                       TileMax* __restrict__ table)
{
    const int n_tiles = ntx * nty * ntz;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        float v; int i;
        tile_argmax(g, gx, gy, gz, t / (nty * ntz), (t / ntz) % nty, t % ntz, v, i);
        if (threadIdx.x == 0) table[t] = TileMax{v, i};
        __syncthreads();
    }
}

// np.mean of a float32 slice of n (1..128) cells: pairwise_sum's base case (a running sum below 8 elements; else eight interleaved
// partial sums combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the rest in order), one float32 divide
__device__ float np_mean(const float* __restrict__ p, int64_t stride, int n)
{
    float s;
    if (n < 8) {
        s = 0.f;
        for (int k = 0; k < n; ++k) s += p[k * stride];
    } else {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = p[j * stride];
        const int n8 = n - n % 8;
        for (int k = 8; k < n8; k += 8)
            for (int j = 0; j < 8; ++j) r[j] += p[(k + j) * stride];
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int k = n8; k < n; ++k) s += p[k * stride];
    }
    return s / (float)n;
}

// edge k of the box, in the notebook's order: 0-3 along axis 0 at (y, z) = (l,l) (l,r) (r,l) (r,r); 4-7 along axis 1 at (x, z);
// 8-11 along axis 2 at (x, y); slices half-open [lll, rrr)
__device__ float edge_mean(const float* __restrict__ g, int gy, int gz, const int* l, const int* r, int k)
{
    const int a = (k >> 1) & 1, b = k & 1;
    int x, y, z, n;
    int64_t stride;
    if (k < 4) { x = l[0]; y = a ? r[1] : l[1]; z = b ? r[2] : l[2]; n = r[0] - l[0]; stride = (int64_t)gy * gz; }
    else if (k < 8) { x = a ? r[0] : l[0]; y = l[1]; z = b ? r[2] : l[2]; n = r[1] - l[1]; stride = gz; }
    else { x = a ? r[0] : l[0]; y = b ? r[1] : l[1]; z = l[2]; n = r[2] - l[2]; stride = 1; }
    return np_mean(g + ((int64_t)x * gy + y) * gz + z, stride, n);
}

__global__ __launch_bounds__(SCN_LOOP_THREADS) void proposals_loop_kernel(float* __restrict__ g, int gx, int gy, int gz,
                                                                          TileMax* __restrict__ table, int ntx, int nty, int ntz,
                                                                          float thresh, int margin, int max_props, int max_iters,
                                                                          int32_t* __restrict__ loc_out, float* __restrict__ val_out,
                                                                          float* __restrict__ diff_out, int32_t* __restrict__ count_out)
{
    __shared__ float means[12];
    const int tid = threadIdx.x;
    const int n_tiles = ntx * nty * ntz;
    int count = 0, prev_i = -1;
    bool have_max = false;
    float max_val = 0.f, prev_diff = 0.f;
    for (int it = 0; it < max_iters && count < max_props; ++it) {
        // loc = first arg-max of the (suppressed) grid, from the tile table
        float v = -INFINITY; int i = INT32_MAX;
        for (int t = tid; t < n_tiles; t += blockDim.x) {
            const TileMax e = table[t];
            if (better(e.v, e.i, v, i)) { v = e.v; i = e.i; }
        }
        block_argmax(v, i);
        const int loc[3] = {i / (gy * gz), (i / gz) % gy, i % gz};
        const int dims[3] = {gx, gy, gz};
        int l[3], r[3];
        for (int a = 0; a < 3; ++a) { l[a] = max(0, loc[a] - margin); r[a] = min(dims[a] - 1, loc[a] + margin); }
        if (tid < 12) means[tid] = edge_mean(g, gy, gz, l, r, tid);
        __syncthreads();
        float s = means[0];
        for (int k = 1; k < 12; ++k) s += means[k];
        const float diff = v - s / 12.f;
        __syncthreads();                                     // (means is rewritten by the next iteration)
        // from here on the notebook would repeat this iteration forever: its proposals are emitted once
        if (i == prev_i && __float_as_uint(diff) == __float_as_uint(prev_diff)) break;
        prev_i = i; prev_diff = diff;
        if (diff > thresh) {
            if (!have_max) { max_val = diff; have_max = true; }
            if (tid == 0) {
                loc_out[3 * count] = loc[0]; loc_out[3 * count + 1] = loc[1]; loc_out[3 * count + 2] = loc[2];
                val_out[count] = v;
                diff_out[count] = diff;
            }
            ++count;
        }
        if (diff < thresh || (have_max && diff < max_val * 0.7f)) break;
        // smoothed_grid[lll:rrr, lll:rrr, lll:rrr] = 0, then the tiles the box touches are recomputed
        const int bx = r[0] - l[0], by = r[1] - l[1], bz = r[2] - l[2];
        const int n_box = bx * by * bz;
        for (int k = tid; k < n_box; k += blockDim.x) {
            const int x = l[0] + k / (by * bz), y = l[1] + (k / bz) % by, z = l[2] + k % bz;
            g[((int64_t)x * gy + y) * gz + z] = 0.f;
        }
        __threadfence();
        __syncthreads();
        if (n_box > 0) {
            for (int tx = l[0] / SCN_TILE; tx <= (r[0] - 1) / SCN_TILE; ++tx)
                for (int ty = l[1] / SCN_TILE; ty <= (r[1] - 1) / SCN_TILE; ++ty)
                    for (int tz = l[2] / SCN_TILE; tz <= (r[2] - 1) / SCN_TILE; ++tz) {
                        float tv; int ti;
                        tile_argmax(g, gx, gy, gz, tx, ty, tz, tv, ti);
                        if (tid == 0) table[(tx * nty + ty) * ntz + tz] = TileMax{tv, ti};
                    }
        }
        __threadfence();
        __syncthreads();
    }
    if (tid == 0) *count_out = count;
}

__global__ void zero_count_kernel(int32_t* count) { if (threadIdx.x == 0) *count = 0; }

static void tiles_of(int gx, int gy, int gz, int* ntx, int* nty, int* ntz)
{
    *ntx = (gx + SCN_TILE - 1) / SCN_TILE; *nty = (gy + SCN_TILE - 1) / SCN_TILE; *ntz = (gz + SCN_TILE - 1) / SCN_TILE;
}

extern "C" size_t cppf_scene_proposals_workspace_bytes(int gx, int gy, int gz)
{
    if (gx < 1 || gy < 1 || gz < 1) return 0;
    int ntx, nty, ntz;
    tiles_of(gx, gy, gz, &ntx, &nty, &ntz);
    return 2 * align256((size_t)gx * gy * gz * sizeof(float)) + align256((size_t)ntx * nty * ntz * sizeof(TileMax));
}

extern "C" int cppf_scene_proposals(const float* grid, int gx, int gy, int gz, const double* weights, int radius, float thresh,
                                    int margin, int max_proposals, int max_iters, int32_t* loc, float* value, float* diff,
                                    int32_t* count, float* smoothed_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!grid || !loc || !value || !diff || !count || gx < 1 || gy < 1 || gz < 1) return CPPF_EINVAL;
    if (margin < 1 || margin > SCN_MAX_MARGIN || max_proposals < 0 || max_iters < 0) return CPPF_EINVAL;
    if ((int64_t)gx * gy * gz >= ((int64_t)1 << 30)) return CPPF_EUNSUPPORTED;     // flat indices are int32
    GaussWeights W;
    if (int rc = check_weights(weights, radius, &W)) return rc;
    if (!workspace || workspace_bytes < cppf_scene_proposals_workspace_bytes(gx, gy, gz)) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t gb = align256((size_t)gx * gy * gz * sizeof(float));
    float* a = static_cast<float*>(workspace);
    float* b = reinterpret_cast<float*>(static_cast<char*>(workspace) + gb);
    TileMax* table = reinterpret_cast<TileMax*>(static_cast<char*>(workspace) + 2 * gb);
    if (int rc = gauss3(grid, a, b, smoothed_out, gx, gy, gz, W, radius, st)) return rc;
    if (gx < 2 || gy < 2 || gz < 2) {                  // empty edge slices: the notebook's NaN / TypeError; defined as no proposals
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(64), 0, st, count);
        CPPF_CHECK_LAUNCH();
        return 0;
    }
    int ntx, nty, ntz;
    tiles_of(gx, gy, gz, &ntx, &nty, &ntz);
    const int n_tiles = ntx * nty * ntz;
    hipLaunchKernelGGL(tile_max_kernel, dim3(n_tiles < 16384 ? n_tiles : 16384), dim3(256), 0, st, a, gx, gy, gz, ntx, nty, ntz, table);
    hipLaunchKernelGGL(proposals_loop_kernel, dim3(1), dim3(SCN_LOOP_THREADS), 0, st, a, gx, gy, gz, table, ntx, nty, ntz, thresh,
                       margin, max_proposals, max_iters, loc, value, diff, count);
    CPPF_CHECK_LAUNCH();
    return 0;
}

// ----------------------------------------------------------------------------- pair filter (cell 6)
// keep[p] = !(|n1.n2| > 0.9 & |ab.n1| < 0.1 & |ab.n2| < 0.1), ab = (a - b) / (||a - b|| + 1e-7), float32 as numpy computes it
// (three-term sums left to right).  A pair with an endpoint outside [0, n_points) is dropped.
__global__ __launch_bounds__(256) void pair_filter_kernel(const float* __restrict__ pc, const float* __restrict__ nrm,
                                                          const void* __restrict__ idxs, int idx_is_i64, int64_t n_points,
                                                          int64_t n_pairs, uint8_t* __restrict__ keep)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t ia, ib;
        if (idx_is_i64) { ia = static_cast<const int64_t*>(idxs)[2 * p]; ib = static_cast<const int64_t*>(idxs)[2 * p + 1]; }
        else { ia = static_cast<const int32_t*>(idxs)[2 * p]; ib = static_cast<const int32_t*>(idxs)[2 * p + 1]; }
        if (ia < 0 || ib < 0 || ia >= n_points || ib >= n_points) { keep[p] = 0; continue; }
        const f3 n1 = ld3(nrm, (int)ia), n2 = ld3(nrm, (int)ib);
        const f3 ab = sub3(ld3(pc, (int)ia), ld3(pc, (int)ib));
        const float den = sqrtf((ab.x * ab.x + ab.y * ab.y) + ab.z * ab.z) + 1e-7f;
        const f3 u = {ab.x / den, ab.y / den, ab.z / den};
        const float c0 = (n1.x * n2.x + n1.y * n2.y) + n1.z * n2.z;
        const float c1 = (u.x * n1.x + u.y * n1.y) + u.z * n1.z;
        const float c2 = (u.x * n2.x + u.y * n2.y) + u.z * n2.z;
        keep[p] = (fabsf(c0) > 0.9f && fabsf(c1) < 0.1f && fabsf(c2) < 0.1f) ? 0 : 1;
    }
}

// at most 16 384 workgroups of 256 lanes (tested: 4 194 304 + 333 pairs, every lane on its second trip or in the ragged tail)

extern "C" int cppf_pair_filter_distinct(const float* pc, const float* nrm, const void* point_idxs, int idx_is_i64, int64_t n_points,
                                         int64_t n_pairs, uint8_t* keep, void* stream)
{
    if (!pc || !nrm || !point_idxs || !keep || n_points < 0 || n_points > INT32_MAX || n_pairs < 0) return CPPF_EINVAL;
    if (n_pairs == 0) return 0;
    hipLaunchKernelGGL(pair_filter_kernel, dim3(blocks256(n_pairs)), dim3(256), 0, (hipStream_t)stream, pc, nrm, point_idxs,
                       idx_is_i64, n_points, n_pairs, keep);
    CPPF_CHECK_LAUNCH();
    return 0;
}

// ----------------------------------------------------------------------------- instance segmentation (cell 11)
// contrib[n] = how often point n is an endpoint of a back-vote survivor (integer atomics: the same counts on every run)
__global__ __launch_bounds__(256) void endpoint_hist_kernel(const int32_t* __restrict__ idx, const uint8_t* __restrict__ surv,
                                                            int64_t n_pairs, int64_t n_points, int32_t* __restrict__ contrib)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        if (!surv[p]) continue;
        const int2 ij = reinterpret_cast<const int2*>(idx)[p];
        if (ij.x >= 0 && ij.x < n_points) atomicAdd(contrib + ij.x, 1);
        if (ij.y >= 0 && ij.y < n_points) atomicAdd(contrib + ij.y, 1);
    }
}

__global__ __launch_bounds__(256) void point_mask_kernel(const int32_t* __restrict__ contrib, int64_t n_points, int min_contrib,
                                                         uint8_t* __restrict__ point_mask)
{
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < n_points; n += (int64_t)gridDim.x * blockDim.x)
        point_mask[n] = contrib[n] > min_contrib ? 1 : 0;
}

// a survivor is kept when either endpoint is in the instance
__global__ __launch_bounds__(256) void pair_keep_kernel(const int32_t* __restrict__ idx, const uint8_t* __restrict__ surv,
                                                        int64_t n_pairs, int64_t n_points, const uint8_t* __restrict__ point_mask,
                                                        uint8_t* __restrict__ keep)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        uint8_t k = 0;
        if (surv[p]) {
            const int2 ij = reinterpret_cast<const int2*>(idx)[p];
            const bool a = ij.x >= 0 && ij.x < n_points && point_mask[ij.x];
            const bool b = ij.y >= 0 && ij.y < n_points && point_mask[ij.y];
            k = (a || b) ? 1 : 0;
        }
        keep[p] = k;
    }
}

extern "C" size_t cppf_segment_instance_workspace_bytes(int64_t n_points, int64_t n_pairs)
{
    if (n_points < 0 || n_pairs < 0) return 0;
    return align256((size_t)n_points * sizeof(int32_t)) + align256((size_t)n_pairs) + cppf_compact_workspace_bytes(n_pairs);
}

extern "C" int cppf_segment_instance(const int32_t* point_idxs, const uint8_t* surv_mask, int64_t n_pairs, int64_t n_points,
                                     int min_contrib, uint8_t* point_mask, int32_t* pairs_out, int32_t* count, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    if (!point_idxs || !surv_mask || !point_mask || !pairs_out || !count || n_pairs < 0 || n_points < 1 || n_points > INT32_MAX)
        return CPPF_EINVAL;
    if (!workspace || workspace_bytes < cppf_segment_instance_workspace_bytes(n_points, n_pairs)) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* contrib = static_cast<int32_t*>(workspace);
    const size_t cb = align256((size_t)n_points * sizeof(int32_t));
    uint8_t* keep = static_cast<uint8_t*>(workspace) + cb;
    void* cws = static_cast<char*>(workspace) + cb + align256((size_t)n_pairs);
    const size_t cws_bytes = workspace_bytes - cb - align256((size_t)n_pairs);
    if (hipError_t e = hipMemsetAsync(contrib, 0, (size_t)n_points * sizeof(int32_t), st)) return (int)e;
    if (n_pairs > 0)
        hipLaunchKernelGGL(endpoint_hist_kernel, dim3(blocks256(n_pairs)), dim3(256), 0, st, point_idxs, surv_mask, n_pairs,
                           n_points, contrib);
    hipLaunchKernelGGL(point_mask_kernel, dim3(blocks256(n_points)), dim3(256), 0, st, contrib, n_points, min_contrib, point_mask);
    if (n_pairs > 0)
        hipLaunchKernelGGL(pair_keep_kernel, dim3(blocks256(n_pairs)), dim3(256), 0, st, point_idxs, surv_mask, n_pairs, n_points,
                           point_mask, keep);
    CPPF_CHECK_LAUNCH();
    if (n_pairs == 0) {
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(64), 0, st, count);
        CPPF_CHECK_LAUNCH();
        return 0;
    }
    return cppf_compact_mask(keep, n_pairs, pairs_out, count, cws, cws_bytes, stream);
}
