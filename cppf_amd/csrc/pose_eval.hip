// NOCS pose evaluation on gfx950 (MI355X): the box IoU, the degree / centimetre errors and the two greedy matchings of
// cppf_amd/evaluation.py (utils/util.py:181-255,342-416,470-517 of the reference).  C ABI, the arithmetic and the tie rules:
// include/cppf.h ("Pose evaluation").  All arithmetic is fp64 in evaluation.py's order, without contraction.
//
// cppf_pose_eval_pairs:
//   pe_scan_kernel   one 1024-lane workgroup: item_off[p] = the first work item of pair p (20 items for a swept pair, 1 otherwise),
//                    item_off[M] = their number; iou <- 0
//   pe_pairs_kernel  one lane per work item (pair, rotation k): the IoU of box 1 turned by k * 18 degrees about its y axis with
//                    box 2; a swept pair's IoU is the maximum over its items (a 64-bit integer max on the bits of a non-negative
//                    double: exact in any order); item k = 0 also writes the pair's errors.
//                    The clipped polygon (<= 10 vertices: a quad cut by six planes) lives in LDS, two buffers per lane
//                    ([buffer][vertex][coordinate][lane]: a lane's slots are in its own banks whatever vertex it indexes), the
//                    two box frames live in registers behind fully unrolled axis loops: no dynamically indexed private array.
// cppf_pose_eval_match_iou / _match_pose: one lane per (group, threshold) / (group, degree threshold, shift threshold); a group's
//   claimed ground truths are a u32 mask.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"
#include "pose_eval_box.h"     // PE_LANES, PE_MAXV, PeFrame, pe_det3, pe_frame, pe_clip, pe_flux, pe_volume, pe_iou

#define PE_SYM 20              // rotations of the up-symmetry sweep (utils/util.py:200-209)
#define PE_SCAN_THREADS 1024
#define PE_MATCH_THREADS 256
#define PE_MAX_BLOCKS 8192     // x PE_LANES = 524 288 work items per trip of the stride loop (tested: 540 000 items, and a swept
                               // pair whose 20 items cross the trip boundary -- tests/test_gpu_limits.py)
#define PE_GROUP_CAP 32        // predictions / ground truths of one group (CPPF_POSE_EVAL_GROUP_CAP)

static_assert(PE_GROUP_CAP == CPPF_POSE_EVAL_GROUP_CAP, "the claimed set is one u32");

// cos / sin of 2 pi k / 20 as the host's math.cos / math.sin return them (evaluation._rot_y)
__constant__ double pe_cos[PE_SYM] = {
    0x1.0000000000000p+0, 0x1.e6f0e134454ffp-1, 0x1.9e3779b97f4a8p-1, 0x1.2cf2304755a5ep-1, 0x1.3c6ef372fe950p-2,
    0x1.1a62633145c07p-54, -0x1.3c6ef372fe94ep-2, -0x1.2cf2304755a5dp-1, -0x1.9e3779b97f4a7p-1, -0x1.e6f0e134454ffp-1,
    -0x1.0000000000000p+0, -0x1.e6f0e13445501p-1, -0x1.9e3779b97f4a9p-1, -0x1.2cf2304755a5fp-1, -0x1.3c6ef372fe952p-2,
    -0x1.a79394c9e8a0ap-53, 0x1.3c6ef372fe94cp-2, 0x1.2cf2304755a5cp-1, 0x1.9e3779b97f4a7p-1, 0x1.e6f0e134454ffp-1};
__constant__ double pe_sin[PE_SYM] = {
    0x0.0p+0, 0x1.3c6ef372fe94fp-2, 0x1.2cf2304755a5ep-1, 0x1.9e3779b97f4a8p-1, 0x1.e6f0e134454ffp-1,
    0x1.0000000000000p+0, 0x1.e6f0e13445500p-1, 0x1.9e3779b97f4a8p-1, 0x1.2cf2304755a5fp-1, 0x1.3c6ef372fe951p-2,
    0x1.1a62633145c07p-53, -0x1.3c6ef372fe946p-2, -0x1.2cf2304755a5dp-1, -0x1.9e3779b97f4a7p-1, -0x1.e6f0e134454ffp-1,
    -0x1.0000000000000p+0, -0x1.e6f0e13445500p-1, -0x1.9e3779b97f4a9p-1, -0x1.2cf2304755a60p-1, -0x1.3c6ef372fe953p-2};

static inline size_t pe_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------------------ work items
__global__ __launch_bounds__(PE_SCAN_THREADS) void pe_scan_kernel(const int32_t* __restrict__ sweep, int64_t M,
                                                                  int32_t* __restrict__ item_off, double* __restrict__ iou)
{
    __shared__ int32_t part[PE_SCAN_THREADS];
    const int64_t K = (M + PE_SCAN_THREADS - 1) / PE_SCAN_THREADS;
    const int64_t t0 = min(M, (int64_t)threadIdx.x * K), t1 = min(M, t0 + K);
    int32_t s = 0;
    for (int64_t t = t0; t < t1; ++t) {
        s += sweep[t] ? PE_SYM : 1;
        iou[t] = 0.0;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t b = 0;
        for (int l = 0; l < PE_SCAN_THREADS; ++l) {
            const int32_t T = part[l];
            part[l] = b;
            b += T;
        }
        item_off[M] = b;
    }
    __syncthreads();
    int32_t c = part[threadIdx.x];
    for (int64_t t = t0; t < t1; ++t) {
        item_off[t] = c;
        c += sweep[t] ? PE_SYM : 1;
    }
}

// the pair that owns work item `it`: the last p with off[p] <= it (off increasing, off[0] = 0 <= it < off[M])
__device__ __forceinline__ int64_t pe_owner(const int32_t* __restrict__ off, int64_t M, int32_t it)
{
    int64_t lo = 0, hi = M - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= it) lo = mid; else hi = mid - 1;
    }
    return lo;
}


__global__ __launch_bounds__(PE_LANES) void pe_pairs_kernel(const double* __restrict__ pred_RT, const double* __restrict__ pred_scales,
                                                            int64_t n_pred, const double* __restrict__ gt_RT,
                                                            const double* __restrict__ gt_scales, const int32_t* __restrict__ gt_up_sym,
                                                            int64_t n_gt, const int32_t* __restrict__ pairs,
                                                            const int32_t* __restrict__ sweep, int64_t M,
                                                            const int32_t* __restrict__ item_off, double* __restrict__ iou,
                                                            double* __restrict__ err)
{
    __shared__ double poly[2 * PE_MAXV * 3 * PE_LANES];
    double* buf = poly + threadIdx.x;
    const int32_t total = item_off[M];
    for (int64_t it = (int64_t)blockIdx.x * PE_LANES + threadIdx.x; it < total; it += (int64_t)gridDim.x * PE_LANES) {
        const int64_t p = pe_owner(item_off, M, (int32_t)it);
        const int k = (int)(it - item_off[p]);
        const int64_t ip = pairs[2 * p], ig = pairs[2 * p + 1];
        if (ip < 0 || ip >= n_pred || ig < 0 || ig >= n_gt || k >= PE_SYM) {     // an index outside the arrays: NaN, nothing is read
            if (k == 0) {
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
                iou[p] = nan;
                err[2 * p] = nan;
                err[2 * p + 1] = nan;
            }
            continue;
        }
        const double* m1 = pred_RT + 16 * ip;
        const double* m2 = gt_RT + 16 * ig;
        double R1[3][3], R2[3][3], t1[3], t2[3], s1[3], s2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { R1[r][c] = m1[4 * r + c]; R2[r][c] = m2[4 * r + c]; }
            t1[r] = m1[4 * r + 3];
            t2[r] = m2[4 * r + 3];
            s1[r] = pred_scales[3 * ip + r];
            s2[r] = gt_scales[3 * ig + r];
        }
        if (k == 0) {                                               // evaluation.compute_RT_degree_cm_symmetry
            const double q1 = cbrt(pe_det3(R1)), q2 = cbrt(pe_det3(R2));
            double cosv;
            if (gt_up_sym[ig]) {
                const double a0 = R1[0][1] / q1, a1 = R1[1][1] / q1, a2 = R1[2][1] / q1;
                const double b0 = R2[0][1] / q2, b1 = R2[1][1] / q2, b2 = R2[2][1] / q2;
                cosv = ((a0 * b0 + a1 * b1) + a2 * b2) / (sqrt((a0 * a0 + a1 * a1) + a2 * a2) * sqrt((b0 * b0 + b1 * b1) + b2 * b2));
            } else {
                double tr = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    tr += ((R1[r][0] / q1) * (R2[r][0] / q2) + (R1[r][1] / q1) * (R2[r][1] / q2)) + (R1[r][2] / q1) * (R2[r][2] / q2);
                cosv = (tr - 1.0) / 2.0;
            }
            const double dx = t1[0] - t2[0], dy = t1[1] - t2[1], dz = t1[2] - t2[2];
            err[2 * p] = acos(fmin(1.0, fmax(-1.0, cosv))) * (180.0 / 3.141592653589793);
            err[2 * p + 1] = sqrt((dx * dx + dy * dy) + dz * dz) * 100.0;
        }
        const int sw = sweep[p] != 0;
        if (sw) {                                                   // RT_1 @ _rot_y(2 pi k / 20): columns 0 and 2 turn, k = 0 is exact
            const double c = pe_cos[k], s = pe_sin[k];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double x = R1[r][0], z = R1[r][2];
                R1[r][0] = x * c + z * (-s);
                R1[r][2] = x * s + z * c;
            }
        }
        PeFrame A, B;
        pe_frame(R1, t1, s1, A);
        pe_frame(R2, t2, s2, B);
        const double v = pe_iou(A, B, buf);
        if (sw)
            atomicMax(reinterpret_cast<unsigned long long*>(iou + p), (unsigned long long)__double_as_longlong(v));
        else
            iou[p] = v;
    }
}

extern "C" size_t cppf_pose_eval_pairs_workspace_bytes(int64_t n_pairs)
{
    if (n_pairs < 0 || n_pairs > CPPF_POSE_EVAL_MAX_PAIRS) return 0;
    return pe_align((size_t)(n_pairs + 1) * sizeof(int32_t));
}

extern "C" int cppf_pose_eval_pairs(const double* pred_RT, const double* pred_scales, int64_t n_pred, const double* gt_RT,
                                    const double* gt_scales, const int32_t* gt_up_sym, int64_t n_gt, const int32_t* pairs,
                                    const int32_t* sweep, int64_t n_pairs, double* iou, double* err, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    if (n_pairs < 0 || n_pairs > CPPF_POSE_EVAL_MAX_PAIRS || n_pred < 0 || n_gt < 0) return CPPF_EINVAL;
    if (n_pairs == 0) return 0;
    if (!pred_RT || !pred_scales || !gt_RT || !gt_scales || !gt_up_sym || !pairs || !sweep || !iou || !err || n_pred < 1 || n_gt < 1)
        return CPPF_EINVAL;
    if (!workspace || workspace_bytes < cppf_pose_eval_pairs_workspace_bytes(n_pairs)) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* item_off = static_cast<int32_t*>(workspace);
    pe_scan_kernel<<<1, PE_SCAN_THREADS, 0, st>>>(sweep, n_pairs, item_off, iou);
    const int64_t need = (n_pairs * PE_SYM + PE_LANES - 1) / PE_LANES;
    const unsigned grid = (unsigned)(need < PE_MAX_BLOCKS ? need : PE_MAX_BLOCKS);
    pe_pairs_kernel<<<grid, PE_LANES, 0, st>>>(pred_RT, pred_scales, n_pred, gt_RT, gt_scales, gt_up_sym, n_gt, pairs, sweep, n_pairs,
                                               item_off, iou, err);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ matching
// evaluation.compute_3d_matches for one (group, threshold): predictions in the given (descending score) order take the unclaimed
// ground truth with the highest float32 IoU -- the higher index among equals -- when that IoU is strictly above the threshold.
// (The host walks a prediction's ground truths in descending IoU, skips the claimed ones and stops at the first below the
// threshold: the first unclaimed one decides, one equal to the threshold is passed over and everything after it is no larger.)
__global__ __launch_bounds__(PE_MATCH_THREADS) void pe_match_iou_kernel(const double* __restrict__ iou, const int32_t* __restrict__ pred_off,
                                                                        const int32_t* __restrict__ gt_off,
                                                                        const int64_t* __restrict__ pair_off, int n_groups,
                                                                        const double* __restrict__ thr, int n_thr, int64_t n_pred,
                                                                        int64_t n_gt, int64_t n_pairs, int32_t* __restrict__ pred_match,
                                                                        int32_t* __restrict__ gt_match)
{
    const int64_t idx = (int64_t)blockIdx.x * PE_MATCH_THREADS + threadIdx.x;
    if (idx >= (int64_t)n_groups * n_thr) return;
    const int g = (int)(idx / n_thr), t = (int)(idx % n_thr);
    const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
    if (p0 < 0 || np < 0 || g0 < 0 || ng < 0 || p0 + (int64_t)np > n_pred || g0 + (int64_t)ng > n_gt) return;
    int32_t* pm = pred_match + (int64_t)t * n_pred + p0;
    int32_t* gm = gt_match + (int64_t)t * n_gt + g0;
    for (int j = 0; j < ng; ++j) gm[j] = -1;
    for (int i = 0; i < np; ++i) pm[i] = -1;
    if (np > PE_GROUP_CAP || ng > PE_GROUP_CAP || pair_off[g] < 0 || pair_off[g] + (int64_t)np * ng > n_pairs) return;
    const double* v = iou + pair_off[g];
    const double th = thr[t];
    uint32_t claimed = 0;
    for (int i = 0; i < np; ++i) {
        int best = -1;
        float bv = 0.f;
        for (int j = 0; j < ng; ++j) {
            if ((claimed >> j) & 1u) continue;
            const float o = (float)v[(int64_t)i * ng + j];
            if (best < 0 || o >= bv) { best = j; bv = o; }
        }
        if (best >= 0 && (double)bv > th) {
            claimed |= 1u << best;
            pm[i] = best;
            gm[best] = i;
        }
    }
}

// evaluation.compute_match_from_degree_cm for one (group, degree threshold, shift threshold): every kept prediction takes the
// unclaimed kept ground truth inside both thresholds with the smallest degree + centimetre sum, the lower index among equals.
__global__ __launch_bounds__(PE_MATCH_THREADS) void pe_match_pose_kernel(const double* __restrict__ err, const int32_t* __restrict__ pred_off,
                                                                         const int32_t* __restrict__ gt_off,
                                                                         const int64_t* __restrict__ pair_off, int n_groups,
                                                                         const double* __restrict__ deg_thr, int n_deg,
                                                                         const double* __restrict__ shift_thr, int n_shift,
                                                                         const int32_t* __restrict__ keep_pred,
                                                                         const int32_t* __restrict__ keep_gt, int64_t n_pred, int64_t n_gt,
                                                                         int64_t n_pairs, int32_t* __restrict__ pred_match, int32_t* __restrict__ gt_match)
{
    const int64_t idx = (int64_t)blockIdx.x * PE_MATCH_THREADS + threadIdx.x;
    const int n_ds = n_deg * n_shift;
    if (idx >= (int64_t)n_groups * n_ds) return;
    const int g = (int)(idx / n_ds), ds = (int)(idx % n_ds);
    const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
    if (p0 < 0 || np < 0 || g0 < 0 || ng < 0 || p0 + (int64_t)np > n_pred || g0 + (int64_t)ng > n_gt) return;
    int32_t* pm = pred_match + (int64_t)ds * n_pred + p0;
    int32_t* gm = gt_match + (int64_t)ds * n_gt + g0;
    for (int j = 0; j < ng; ++j) gm[j] = -1;
    for (int i = 0; i < np; ++i) pm[i] = -1;
    if (np > PE_GROUP_CAP || ng > PE_GROUP_CAP || pair_off[g] < 0 || pair_off[g] + (int64_t)np * ng > n_pairs) return;
    const double* e = err + 2 * pair_off[g];
    const double dth = deg_thr[ds / n_shift], sth = shift_thr[ds % n_shift];
    uint32_t claimed = 0;                                         // ground truths that are taken or not kept
    if (keep_gt)
        for (int j = 0; j < ng; ++j)
            if (keep_gt[g0 + j] < 0) claimed |= 1u << j;
    for (int i = 0; i < np; ++i) {
        if (keep_pred && keep_pred[p0 + i] < 0) continue;
        int best = -1;
        double bs = 0.0;
        for (int j = 0; j < ng; ++j) {
            if ((claimed >> j) & 1u) continue;
            const double e0 = e[2 * ((int64_t)i * ng + j)], e1 = e[2 * ((int64_t)i * ng + j) + 1];
            if (e0 > dth || e1 > sth) continue;
            const double sum = e0 + e1;
            if (best < 0 || sum < bs) { best = j; bs = sum; }
        }
        if (best >= 0) {
            claimed |= 1u << best;
            pm[i] = best;
            gm[best] = i;
        }
    }
}

static int pe_match_args(const void* values, const int32_t* pred_off, const int32_t* gt_off, const int64_t* pair_off, int n_groups,
                         int64_t n_cells, int64_t n_pred, int64_t n_gt, int64_t n_pairs, const int32_t* pred_match, const int32_t* gt_match)
{
    if (n_groups < 0 || n_cells < 1 || n_pairs < 0 || n_pred < 0 || n_gt < 0 || n_pred > 0x7fffffffll || n_gt > 0x7fffffffll) return CPPF_EINVAL;
    if (n_groups == 0) return 0;
    if (!pred_off || !gt_off || !pair_off || (n_pred > 0 && !pred_match) || (n_gt > 0 && !gt_match)) return CPPF_EINVAL;
    if (n_pairs > 0 && !values) return CPPF_EINVAL;
    if (((int64_t)n_groups * n_cells + PE_MATCH_THREADS - 1) / PE_MATCH_THREADS > 0x7fffffffll) return CPPF_EINVAL;
    return 1;
}

extern "C" int cppf_pose_eval_match_iou(const double* iou, const int32_t* pred_off, const int32_t* gt_off, const int64_t* pair_off,
                                        int n_groups, const double* thresholds, int n_thresholds, int64_t n_pred, int64_t n_gt,
                                        int64_t n_pairs, int32_t* pred_match, int32_t* gt_match, void* stream)
{
    if (n_thresholds < 1 || !thresholds) return CPPF_EINVAL;
    const int rc = pe_match_args(iou, pred_off, gt_off, pair_off, n_groups, n_thresholds, n_pred, n_gt, n_pairs, pred_match, gt_match);
    if (rc <= 0) return rc;
    const int64_t n = (int64_t)n_groups * n_thresholds;
    pe_match_iou_kernel<<<(unsigned)((n + PE_MATCH_THREADS - 1) / PE_MATCH_THREADS), PE_MATCH_THREADS, 0, (hipStream_t)stream>>>(
        iou, pred_off, gt_off, pair_off, n_groups, thresholds, n_thresholds, n_pred, n_gt, n_pairs, pred_match, gt_match);
    return (int)hipGetLastError();
}

extern "C" int cppf_pose_eval_match_pose(const double* err, const int32_t* pred_off, const int32_t* gt_off, const int64_t* pair_off,
                                         int n_groups, const double* degree_thresholds, int n_degree, const double* shift_thresholds,
                                         int n_shift, const int32_t* keep_pred, const int32_t* keep_gt, int64_t n_pred, int64_t n_gt,
                                         int64_t n_pairs, int32_t* pred_match, int32_t* gt_match, void* stream)
{
    if (n_degree < 1 || n_shift < 1 || n_degree > 32768 || n_shift > 32768 || !degree_thresholds || !shift_thresholds) return CPPF_EINVAL;
    const int rc = pe_match_args(err, pred_off, gt_off, pair_off, n_groups, (int64_t)n_degree * n_shift, n_pred, n_gt, n_pairs, pred_match, gt_match);
    if (rc <= 0) return rc;
    const int64_t n = (int64_t)n_groups * n_degree * n_shift;
    pe_match_pose_kernel<<<(unsigned)((n + PE_MATCH_THREADS - 1) / PE_MATCH_THREADS), PE_MATCH_THREADS, 0, (hipStream_t)stream>>>(
        err, pred_off, gt_off, pair_off, n_groups, degree_thresholds, n_degree, shift_thresholds, n_shift, keep_pred, keep_gt, n_pred, n_gt,
        n_pairs, pred_match, gt_match);
    return (int)hipGetLastError();
}
