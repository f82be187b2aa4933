// Greedy 3D non-maximum suppression over oriented boxes on gfx950 (MI355X), all (image, class) groups of a result set in one call
// (sunrgbd/eval.py:13-35 of the reference; host side and checker: cppf_amd/evaluation.py nms_3d).  C ABI, the rule and the tie
// rule: include/cppf.h ("Box NMS").  The IoU is pose_eval_box.h's pe_iou, the one cppf_pose_eval_pairs runs: same bits.
//
// cppf_box_nms_batch: a memset of the bit matrices, then
//   nms_over_kernel    one lane per unordered pair (i < j) of a group, grid-stride over the pairs of all groups; the owning group is
//                      found in the pair-offset table (the last g with pair_off[g] <= item), (i, j) from the row-by-row position in
//                      the group's upper triangle.  IoU > thresh sets bit j of row i and bit i of row j of the group's bit matrix
//                      (m rows of ceil(m / 64) 64-bit words) with an integer atomicOr: the words do not depend on the order.
//                      The clipped polygons live in LDS in pe_pairs_kernel's per-lane layout (64 lanes, 30 720 B).
//   nms_greedy_kernel  one wavefront per group: rank of a box = the number of boxes that go before it (higher score, or equal score
//                      and higher index), counted; order[rank] in LDS; then the serial walk, the "removed" bitset spread over the
//                      lanes (lane l holds word l): a box whose bit is clear is picked, and ORs its row into the bitset.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/cppf.h"
#include "pose_eval_box.h"

#define NMS_CAP 1024               // boxes of one group (CPPF_BOX_NMS_GROUP_CAP): 16 words per row, one per lane of a quarter wavefront
#define NMS_WORDS (NMS_CAP / 64)   // (tested: groups of 960, 961, 1023 and 1024 boxes, the refusal at 1025 and one call of 3000
                                   // groups -- tests/test_gpu_limits.py)
#define NMS_MAX_BLOCKS 2048        // nms_over_kernel's grid: 131 072 lanes, a single group of 513 boxes or more enters the stride loop
#define NMS_MAX_PAIRS 0x7fffffffll

static_assert(NMS_CAP == CPPF_BOX_NMS_GROUP_CAP, "a row of the bit matrix is at most one word per lane");
static_assert(NMS_WORDS <= PE_LANES, "the removed set is one word per lane");

static inline size_t nms_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the three tables of a call, 256-byte aligned, then the bit matrices
struct NmsLayout { size_t group_off, pair_off, word_off, bits, total; };

static NmsLayout nms_layout(int64_t n_boxes, int n_groups)
{
    NmsLayout L;
    const size_t G1 = (size_t)n_groups + 1;
    L.group_off = 0;
    L.pair_off = nms_align(G1 * sizeof(int32_t));
    L.word_off = L.pair_off + nms_align(G1 * sizeof(int64_t));
    L.bits = L.word_off + nms_align(G1 * sizeof(int64_t));
    // a group of m boxes has m rows of ceil(m / 64) words, m <= n and m <= NMS_CAP: at most n * min(NMS_WORDS, ceil(n / 64)) words
    const int64_t wpr = (n_boxes + 63) / 64;
    L.total = L.bits + nms_align((size_t)n_boxes * (size_t)(wpr < NMS_WORDS ? wpr : NMS_WORDS) * sizeof(uint64_t));
    return L;
}

// the group that owns pair item `it`: the last g with off[g] <= it (off non-decreasing, off[0] = 0 <= it < off[G]; a group without
// pairs has off[g] == off[g + 1] and is passed over)
__device__ __forceinline__ int nms_owner(const int64_t* __restrict__ off, int G, int64_t it)
{
    int lo = 0, hi = G - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= it) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(PE_LANES) void nms_over_kernel(const double* __restrict__ RT, const double* __restrict__ scales,
                                                            const int32_t* __restrict__ group_off, const int64_t* __restrict__ pair_off,
                                                            const int64_t* __restrict__ word_off, int n_groups, double thresh,
                                                            unsigned long long* __restrict__ bits, double* __restrict__ iou_out)
{
    __shared__ double poly[2 * PE_MAXV * 3 * PE_LANES];
    double* buf = poly + threadIdx.x;
    const int64_t total = pair_off[n_groups];
    for (int64_t it = (int64_t)blockIdx.x * PE_LANES + threadIdx.x; it < total; it += (int64_t)gridDim.x * PE_LANES) {
        const int g = nms_owner(pair_off, n_groups, it);
        const int64_t base = group_off[g];
        const int m = group_off[g + 1] - group_off[g];
        const int q = (int)(it - pair_off[g]);                     // position in the upper triangle, row by row: row i starts at
        // i (2m - i - 1) / 2.  The root of that quadratic, then at most a step either way (m <= 1024: every value is exact in fp64)
        const double b2 = (double)(2 * m - 1);
        int i = (int)((b2 - sqrt(b2 * b2 - 8.0 * (double)q)) * 0.5);
        i = i < 0 ? 0 : (i > m - 2 ? m - 2 : i);
        while (i > 0 && i * (2 * m - i - 1) / 2 > q) --i;
        while (i < m - 2 && (i + 1) * (2 * m - i - 2) / 2 <= q) ++i;
        const int j = i + 1 + (q - i * (2 * m - i - 1) / 2);
        if (m < 2 || j <= i || j >= m) continue;                   // (cannot happen for a table the host built; nothing is read)
        const double* m1 = RT + 16 * (base + i);
        const double* m2 = RT + 16 * (base + j);
        double R1[3][3], R2[3][3], t1[3], t2[3], s1[3], s2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { R1[r][c] = m1[4 * r + c]; R2[r][c] = m2[4 * r + c]; }
            t1[r] = m1[4 * r + 3];
            t2[r] = m2[4 * r + 3];
            s1[r] = scales[3 * (base + i) + r];
            s2[r] = scales[3 * (base + j) + r];
        }
        PeFrame A, B;
        pe_frame(R1, t1, s1, A);
        pe_frame(R2, t2, s2, B);
        const double v = pe_iou(A, B, buf);
        if (iou_out) iou_out[it] = v;
        if (v > thresh) {                                          // (NaN compares false: it suppresses nothing)
            const int wpr = (m + 63) >> 6;
            unsigned long long* rows = bits + word_off[g];
            atomicOr(rows + (int64_t)i * wpr + (j >> 6), 1ull << (j & 63));
            atomicOr(rows + (int64_t)j * wpr + (i >> 6), 1ull << (i & 63));
        }
    }
}

__global__ __launch_bounds__(PE_LANES) void nms_greedy_kernel(const double* __restrict__ scores, const int32_t* __restrict__ group_off,
                                                              const int64_t* __restrict__ word_off,
                                                              const unsigned long long* __restrict__ bits, int32_t* __restrict__ pick,
                                                              int32_t* __restrict__ n_pick)
{
    __shared__ double sc[NMS_CAP];
    __shared__ int32_t order[NMS_CAP];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int64_t base = group_off[g];
    int m = group_off[g + 1] - group_off[g];
    m = m < 0 ? 0 : (m > NMS_CAP ? NMS_CAP : m);                   // (the host refused anything else)
    for (int b = lane; b < m; b += PE_LANES) {
        sc[b] = scores[base + b];
        order[b] = -1;                                             // a slot no rank claims (NaN scores: the caller's duty) is skipped
    }
    __syncthreads();
    for (int b = lane; b < m; b += PE_LANES) {                     // rank by (score descending, index descending), by counting
        const double s = sc[b];
        int r = 0;
        for (int c = 0; c < m; ++c) {
            const double o = sc[c];
            r += (o > s || (o == s && c > b)) ? 1 : 0;
        }
        order[r] = b;                                              // r < m
    }
    __syncthreads();
    const int wpr = (m + 63) >> 6;
    const unsigned long long* rows = bits + word_off[g];
    unsigned long long removed = 0;                                // word `lane` of the removed set (lanes >= wpr: unused)
    int np = 0;
    for (int t = 0; t < m; ++t) {
        const int b = order[t];
        if (b < 0) continue;
        const unsigned long long w = __shfl(removed, b >> 6, PE_LANES);
        if ((w >> (b & 63)) & 1ull) continue;                      // (wave-uniform: every lane read the same word)
        if (lane < wpr) removed |= rows[(int64_t)b * wpr + lane];
        if (lane == 0) pick[base + np] = b;
        ++np;
    }
    for (int b = np + lane; b < m; b += PE_LANES) pick[base + b] = -1;
    if (lane == 0) n_pick[g] = np;
}

extern "C" size_t cppf_box_nms_workspace_bytes(int64_t n_boxes, int n_groups)
{
    if (n_boxes < 0 || n_groups < 0 || n_boxes > 0x7fffffffll) return 0;
    return nms_layout(n_boxes, n_groups).total;
}

extern "C" int cppf_box_nms_batch(const double* RT, const double* scales, const double* scores, int64_t n_boxes,
                                  const int32_t* group_off_host, int n_groups, double thresh, int32_t* pick, int32_t* n_pick,
                                  double* iou_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (n_boxes < 0 || n_groups < 0 || n_boxes > 0x7fffffffll) return CPPF_EINVAL;
    if (n_boxes == 0 || n_groups == 0) return 0;
    if (!RT || !scales || !scores || !group_off_host || !pick || !n_pick) return CPPF_EINVAL;
    if (group_off_host[0] != 0 || group_off_host[n_groups] != n_boxes) return CPPF_EINVAL;
    for (int g = 0; g < n_groups; ++g)
        if (group_off_host[g + 1] < group_off_host[g]) return CPPF_EINVAL;
    const size_t G1 = (size_t)n_groups + 1;
    std::vector<int64_t> tab(2 * G1);                              // pair offsets, then bit-matrix word offsets
    int64_t pairs = 0, words = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t m = group_off_host[g + 1] - group_off_host[g];
        if (m > NMS_CAP) return CPPF_EUNSUPPORTED;
        tab[g] = pairs;
        tab[G1 + g] = words;
        pairs += m * (m - 1) / 2;
        words += m * ((m + 63) / 64);
        if (pairs > NMS_MAX_PAIRS) return CPPF_EUNSUPPORTED;
    }
    tab[n_groups] = pairs;
    tab[G1 + n_groups] = words;
    const NmsLayout L = nms_layout(n_boxes, n_groups);
    if (!workspace || workspace_bytes < L.total || L.bits + (size_t)words * sizeof(uint64_t) > L.total) return CPPF_EWORKSPACE;

    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    // small pageable tables: the copies have left the host buffers when the calls return (as cppf_raster_instances' tables)
    hipError_t e = hipMemcpyAsync(ws + L.group_off, group_off_host, G1 * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + L.pair_off, tab.data(), G1 * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + L.word_off, tab.data() + G1, G1 * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && words > 0) e = hipMemsetAsync(ws + L.bits, 0, (size_t)words * sizeof(uint64_t), st);
    if (e != hipSuccess) return (int)e;
    const int32_t* group_off = reinterpret_cast<const int32_t*>(ws + L.group_off);
    const int64_t* pair_off = reinterpret_cast<const int64_t*>(ws + L.pair_off);
    const int64_t* word_off = reinterpret_cast<const int64_t*>(ws + L.word_off);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(ws + L.bits);
    if (pairs > 0) {
        const int64_t need = (pairs + PE_LANES - 1) / PE_LANES;
        const unsigned grid = (unsigned)(need < NMS_MAX_BLOCKS ? need : NMS_MAX_BLOCKS);
        nms_over_kernel<<<grid, PE_LANES, 0, st>>>(RT, scales, group_off, pair_off, word_off, n_groups, thresh, bits, iou_out);
    }
    nms_greedy_kernel<<<(unsigned)n_groups, PE_LANES, 0, st>>>(scores, group_off, word_off, bits, pick, n_pick);
    return (int)hipGetLastError();
}
