/*
 * cppf.h -- C ABI of libcppf_hip.so: the MI355X (gfx950) implementation of CPPF's
 * point-pair-feature -> pair-MLP -> vote -> argmax hot path.
 *
 * This is the drop-in boundary.  The reference (qq456cvb/CPPF) has no FFI of its own: its
 * scripts call three CuPy RawKernels and one torch module directly.  Each entry point below
 * names the reference interface it replaces (paths relative to the reference root); the Python
 * binding that mirrors the reference's call convention lives in cppf_amd/models/{voting,model}.py
 * and the stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a BORROWED pointer; `const float* / int* ...` arguments named below as
 *     "device" are HIP device pointers valid on the current device, nothing is copied or kept.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued
 *     asynchronously on it, nothing synchronises.
 *   - return value: 0 on success, a hipError_t value (>0) when a HIP call failed, or a negative
 *     CPPF_E* code for argument errors.  No exceptions cross the ABI.
 *   - outputs follow the reference: caller-allocated, (zero-)initialised by the caller, updated
 *     in place.
 *   - arrays are DENSE, C-ordered, of exactly the element type named, and aligned to their element (the 12-byte rows of points and
 *     normals are read float by float: 4-byte alignment is enough; pair lists, (mu, nu) and the bin uniforms are read a row at a
 *     time: 8 bytes for int32[.,2] / float[.,2], 16 for int64[.,2]) -- the ABI takes no strides; what the Python layer converts or
 *     refuses in front of it is INTEGRATION.md, "Input forms".
 *   - workspaces are caller-provided device scratch; size them with the *_workspace_bytes()
 *     queries.  The library allocates nothing and keeps no global state.
 *   - ONE exception to "plain scratch": the workspace of the centre vote (cppf_vote_argmax*, cppf_ppf_voting, cppf_vote_grid_raw,
 *     and the back-vote entry points that take `vote_workspace`) carries STATE between calls in its first
 *     cppf_vote_workspace_init_bytes() bytes (~15.7 MB): the (cos, sin) rotation table of its last launch, the queue counters
 *     of the binned path, and the "extra plane" (one u64 per grid cell for halo words and fixed-point wrap-arounds) that every
 *     call leaves zero for the next one.  The contract (ABI version 2):
 *       * give the vote a DEDICATED allocation: never hand the same bytes to another entry point between two votes;
 *       * ZERO its first min(cppf_vote_workspace_init_bytes(), size) bytes once, before the first call (one hipMemsetAsync);
 *       * to recycle a block of a shared arena, zero that many bytes again -- zeroing less (the header alone) makes the header
 *         look fresh while foreign bytes sit in the plane, which the next vote would add to the grid.
 *     What the kernels check for themselves: a header that was never initialised (neither zero nor left by a previous call)
 *     makes EVERY call report arg-max -1 / peak NaN until the caller zeroes the block; the rotation-table cache is re-validated
 *     on every launch (stamp + the 72 entries whose value is known) and rebuilt when the check fails.  A launch that gives up
 *     on a valid workspace (a wrap-around log that overflowed under cppf_vote_grid_raw's fixed_bits, or a *_dyn shape record beyond the capacities) reports
 *     -1 / NaN once, clears the plane itself and leaves the workspace ready for the next call.
 */
#ifndef CPPF_H
#define CPPF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPPF_ABI_VERSION 4   /* 2: vote workspace contract (state in its first cppf_vote_workspace_init_bytes() bytes), cppf_vote_grid_raw; 3: batched votes (CppfVoteItem), cppf_pair_mlp_batch_plan;
                              * 4: CppfPoseTailItem assembles the finished pose record on the device (record_out ...), cppf_stage_batch */

#define CPPF_EINVAL (-1)     /* bad argument (null pointer, negative size, n_rots out of range) */
#define CPPF_EWORKSPACE (-2) /* workspace too small / missing */
#define CPPF_EUNSUPPORTED (-3) /* layer shape not supported by any device kernel */
#define CPPF_ENONFINITE (-4) /* a host cloud holds NaN / inf coordinates (cppf_host_grid_shape) */
#define CPPF_ECAPACITY (-5) /* a device-side bound was exceeded (cppf_raster_depth: the bin list); nothing was dropped silently */

int cppf_abi_version(void);
const char* cppf_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * Centre vote.  Replaces the CuPy RawKernel `ppf_kernel` = CUDA `ppf_voting`
 * (models/voting.py:4-67), launched at nocs/inference.py:192-205.
 *   points      device f32[N,3]        outputs  device f32[n_ppfs,2] = (mu, nu)
 *   probs       device f32[N], or NULL for all ones (every caller of the reference passes ones, nocs/inference.py:201:
 *               then nothing is read)              point_idxs device i32[n_ppfs,2]
 *   grid_obj    device f32[gx,gy,gz]   in/out, accumulated (+=) like the reference's atomicAdd
 *   corner      device f32[3]          res, n_rots (1..CPPF_MAX_ROTS), adaptive: as the reference
 *   n_points    N (the reference kernel never needs it; here it bounds the scan for max(probs))
 * The reference's launch geometry (grid, block) is not part of the ABI.
 * Strategy: the grid is cut into tiles that fit LDS (each owning the samples whose floor cell it holds, plus a one-cell halo);
 * every workgroup accumulates one tile for one chunk of pairs -- or, for grids of 4 tiles and more, for one chunk of the
 * tile's queue of (pair, candidate runs) records that a binning kernel filled -- with 32-bit fixed-point LDS atomics
 * (fp32-exact quantum, see csrc/vote.hip); the raw tiles are written to `workspace` and summed AS INTEGERS into grid_obj by a
 * last kernel that also yields the arg-max (cppf_vote_argmax): the grid is the exact sum of the quantised deposits, the same
 * bits on every run.  n_rots > 72 (nocs/inference.py:39 --num_rots) runs ceil(n_rots / 72) passes of the same kernels, pass w voting
 * rotations [72 w, 72 w + 72) of every pair and adding to the grid.  Grids that would need more than 64 tiles fall back to the
 * reference's own formulation with global fp32 atomics.
 * `workspace`: cppf_vote_workspace_bytes() bytes, DEDICATED to the vote and zero on first use (see the note on workspaces at
 * the top and cppf_vote_workspace_init_bytes below).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_MAX_ROTS 360
size_t cppf_vote_workspace_bytes(int64_t n_ppfs, int n_rots, int gx, int gy, int gz);
/* Fixed-point resolution of the LDS accumulation for this problem size: each deposited weight is
 * rounded to a multiple of p2 * 2^-bits, p2 = max(probs) rounded up to a power of two (24 = fp32
 * precision for every problem of practical size; 0 = global fp32 atomics path, no quantisation). */
int cppf_vote_fixed_point_bits(int64_t n_ppfs, int n_rots, int gx, int gy, int gz);
int cppf_ppf_voting(const float* points, const float* outputs, const float* probs, const int32_t* point_idxs,
                    float* grid_obj, const float* corner, float res, int64_t n_points, int64_t n_ppfs, int n_rots,
                    int gx, int gy, int gz, int adaptive, void* workspace, size_t workspace_bytes, void* stream);

/* Same vote, plus the arg-max that the reference takes on the host (nocs/inference.py:207-208:
 * grid_obj.get(); np.argmax -> first maximum in C order).  out_idx: device i64[1] flat index,
 * out_val: device f32[1] peak value (either may be NULL).
 * accumulate is a flags word: bit 0 (CPPF_VOTE_ACCUMULATE) set: grid_obj += votes (the reference's semantics, caller
 * zero-initialises, :196); clear: grid_obj = votes (spares the caller's memset).  CPPF_VOTE_WORKGROUPS(n), n in 64..256, or'ed in:
 * launch at most n vote workgroups instead of one per CU -- a scheduling hint for callers that keep several instances in flight
 * on different streams (every workgroup pays for a 113 KB tile it zeroes, dumps and the reduce kernel reads back, whatever it
 * deposits: at N = 4096, K = 128 with three instances in flight 128 workgroups give +5 % pairs/s, the instance alone runs 7 %
 * longer).  The hint changes the schedule, not the result: the grid is the exact sum of the quantised deposits
 * and, for grids of < 4 LDS tiles, the quantum is that of a 64-wide launch at EVERY width (cppf_vote_fixed_point_bits), so a call at
 * 256, at 128 and as one object of cppf_vote_argmax_batch return the same bits.  Other bits must be zero (CPPF_EINVAL).
 * point_idxs: device i32[n_ppfs,2] (idx_is_i64 == 0, what the reference passes after `.astype(cp.int32)`,
 * nocs/inference.py:202) or the original i64[n_ppfs,2] of np.random.randint (idx_is_i64 != 0; spares the copy). */
#define CPPF_VOTE_ACCUMULATE 1
#define CPPF_VOTE_WORKGROUPS(n) (((n) & 0x1ff) << 8)
int cppf_vote_argmax(const float* points, const float* outputs, const float* probs, const void* point_idxs,
                     int idx_is_i64, float* grid_obj, const float* corner, float res, int64_t n_points, int64_t n_ppfs, int n_rots,
                     int gx, int gy, int gz, int adaptive, int accumulate, long long* out_idx, float* out_val,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same vote as EXACT INTEGERS, for a pair list that is split over several GPUs (BASELINE.json
 * configs[4] "8-GPU shard"; no counterpart in the reference, whose atomicAdd order is whatever the hardware makes it):
 *   grid_raw     device i64[gx,gy,gz]: every cell's sum of deposited quanta (accumulate != 0: added to what is there)
 *   quantum_out  device f32[1]: value of one quantum, p2 * 2^-bits (0: probs held negative / non-finite weights, the
 *                launch accumulated in fp32 and grid_raw is NOT valid)
 *   fixed_bits   0: the launch chooses (as cppf_vote_argmax does); 8..24: every deposit is rounded to p2 * 2^-fixed_bits.
 *                Ranks that vote slices of ONE pair list pass the same value -- cppf_vote_fixed_point_bits() of the WHOLE
 *                list is always safe -- so that the integer sum of their grids is the single-GPU grid bit for bit,
 *                whatever the order of the all-reduce.  More bits than the launch would choose can overflow the
 *                wrap-around log of a workgroup: reported as quantum 0.
 * Needs the tiled integer path (a grid of <= 64 tiles): CPPF_EUNSUPPORTED otherwise; by-value launches only (no `_dyn` form).
 * n_ppfs == 0 (a rank's slice of a short list) is legal: the image is zero (unchanged with accumulate) and the quantum +infinity,
 * which a MIN over the ranks' quanta ignores and cppf_grid_from_raw turns into an all-zero grid.
 * cppf_grid_from_raw: grid[i] = (float)(raw[i] * quantum) -- the one rounding cppf_vote_argmax applies -- then the arg-max
 * (out_idx / out_val may be NULL; workspace as cppf_grid_argmax). */
int cppf_vote_grid_raw(const float* points, const float* outputs, const float* probs, const void* point_idxs, int idx_is_i64,
                       long long* grid_raw, float* quantum_out, const float* corner, float res, int64_t n_points,
                       int64_t n_ppfs, int n_rots, int gx, int gy, int gz, int adaptive, int accumulate, int fixed_bits,
                       void* workspace, size_t workspace_bytes, void* stream);
int cppf_grid_from_raw(const long long* grid_raw, int64_t n, const float* quantum, float* grid, long long* out_idx,
                       float* out_val, void* workspace, size_t workspace_bytes, void* stream);

/* np.argmax(grid, axis=None) on device (nocs/inference.py:208).  n cells; ties -> lowest index.
 * The tie rule is numpy's for signed zeros too: the cells are compared through keys that would order -0 below +0, but every arg-max of
 * this library (this one, cppf_vote_argmax*) first adds a sum of votes, +0 at least, to the cell, and -0 + +0 = +0 -- a -0 and a
 * +0 tie, the first wins, and the value reported (and an accumulated grid) holds +0 (pinned by tests/test_gpu_device_math.py).
 * workspace: >= 16 bytes of device scratch. */
int cppf_grid_argmax(const float* grid, int64_t n, long long* out_idx, float* out_val, void* workspace,
                     size_t workspace_bytes, void* stream);

/* nocs/inference.py:209-210: T = corners[0] + unravel_index(argmax) * res (fp64); idx device i64[1];
 * T64 device f64[3] and/or T32 device f32[3] (the copy the reference hands to backvote, :225).
 * Optional: peak (device f32[1], the arg-max value) and idx_peak_f64 (device f64[2]) -> {(double)idx, (double)peak},
 * so a host can read index, value and T back as one block of doubles. */
int cppf_center_from_argmax(const long long* idx, const float* corner, double res, int gy, int gz, double* T64,
                            float* T32, const float* peak, double* idx_peak_f64, void* stream);

/* np.argmax(counts) (first maximum) and best_dir = sphere_pts[argmax] (nocs/inference.py:283-284) in one launch:
 * counts device i32[n], sphere64 device f64[n,3], best_idx device i64[1] (optional), best_dir device f64[3]. */
int cppf_counts_argmax_select(const int32_t* counts, int n, const double* sphere64, long long* best_idx,
                              double* best_dir, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The pose tail of up to 8 objects -- everything between the centre vote's arg-max and the pose record, nocs/inference.py:209-303,335,
 * for the instances of a frame (:120 loops over them) -- in SIX launches instead of six per object:
 *   1. T = corner + unravel(arg-max) * res (:209-210)  [cppf_pose_tail_begin]     4. second MLP pass on the survivors (:236-256)
 *   2. back-vote filter (:216-231)                     [cppf_backvote_count64]       [cppf_pair_mlp_decode_sel], items with second_pass
 *   3. survivor compaction (:231)                      [cppf_compact_scatter]     5. orientation vote + sphere-bin count (:259-284)
 *                                                                                     [cppf_rot_sphere_count_dirs]
 *                                                                                 6. best_dir, sign and scale sums (:283-301,335) [cppf_pose_sums]
 * Every launch runs the single-object kernel's body on item blockIdx.y of a by-value item array: per object the results are those
 * of the six single calls in brackets, bit for bit.  Buffers are the caller's (cppf_amd.inference.PoseWorkspace lays them out):
 *   rec      device f64[21]: T[3] | best_dir[2][3] | sign sums[2][3] | scale sums[4] | arg-max index, peak -- the pose record
 *   tail0    the region zeroed by launch 1 (16-byte multiple): record, sphere-bin counts, ticket, per-chunk survivor counts
 *   counts   device i32[2][n_sphere] (inside tail0); chunk_counts i32[ceil(n_pairs / 1024)] (inside tail0); ticket u32 (inside tail0)
 *   heads    device f32[n_pairs,8]: rows of the survivors are written by launch 4 (second_pass = 1), or hold every pair's heads
 *            from an all-heads first pass (second_pass = 0)
 *            second_pass = 2: second pass on a bf16 image (`packed` from cppf_pair_mlp_bf16_pack*, launch 4 =
 *            cppf_pair_mlp_bf16_decode_sel_batch); a batch that mixes 1 and 2 is CPPF_EINVAL
 *   mlp_workspace  the per-point table the first pass (cppf_pair_mlp_decode / _batch) left for this object
 * Common to the batch: the pair-encoder architecture (standard fused one only), n_rots, the sphere bins (unit vectors with a monotone y
 * column: fibonacci_sphere; sphere_sorted_by_y = +1 descending / -1 ascending), thr = cos(angle_tol), max_rot_pairs (:277-280).
 * A sums_workspace below cppf_pose_sums_workspace_bytes() or, for an item with second_pass, an mlp_workspace below
 * cppf_pair_mlp_workspace_bytes(n_points, ...) is CPPF_EWORKSPACE, returned before anything is enqueued: no buffer of any item is touched. */
typedef struct CppfPoseTailItem {
    const float* pc; const float* nrm; const float* feat;          /* device f32[n_points,3], f32[n_points,3], f32[n_points,F] */
    const long long* idx64; int32_t* idx32;                         /* pair list i64[n_pairs,2]; its i32 copy (OUTPUT of launch 2).  idx64 NULL:
                                                                     * the list IS idx32 (an INPUT: drawn as int32, cppf_stage_batch) */
    const float* outputs; const float* u_rot; float* heads;         /* (mu, nu) f32[n_pairs,2]; uniforms f32[n_pairs,2]; see above */
    const float* corner; const int32_t* shape_dev;                  /* f32[3]; NULL (dims by value) or device i32[4] {n_points, gx, gy, gz} */
    const long long* argmax_idx; const float* peak;                 /* the vote's outputs */
    const float* packed; void* mlp_workspace; size_t mlp_workspace_bytes;
    const void* vote_workspace;                                     /* the vote's workspace (its cached rotation table) or NULL */
    double* rec; float* T32;
    void* tail0; size_t tail0_bytes;
    uint8_t* mask; int32_t* chunk_counts; int32_t* surv; int32_t* count; int32_t* counts;
    long long* best_idx; unsigned* ticket; void* sums_workspace; size_t sums_workspace_bytes;
    int64_t n_points, n_pairs;
    double res64;                                                   /* res as the caller holds it (fp64: T = corner + cand * res, :210) */
    float res, tol;                                                 /* fp32 res of the kernels; back-vote tolerance (3 * res) */
    int gx, gy, gz, n_dirs, second_pass;
    /* Optional (record_out != NULL): the FINISHED pose record, assembled by launch 6's last workgroup -- the host end of
     * nocs/inference.py:299-339 (axis flips from the sign sums, right axis orthogonalised or derived, scale = exp(mean) * scale_mean * 2) --
     * so that a batch's records enter the end-of-batch gather without a host round trip.
     *   record_out  device f64[16]: T[3] | up[3] | right[3] | scale[3] | arg-max index | peak | survivors | object id
     *   object id = *object_id_dev (device i64, e.g. &CppfStageDesc.object_id) when that is not NULL, else object_id_host
     * A degenerate right axis (|right| < 1e-7, :325-328: the reference draws a random vector) takes the fixed vector
     * numpy.random.default_rng(0).standard_normal(3), as cppf_amd.inference._assemble does.
     * An instance the shape-polymorphic vote refused (arg-max index -1, peak NaN) has no pose: T, up, right and scale of its record
     * are NaN; the arg-max -1, the survivor count and the object id are written as always. */
    double* record_out;
    const long long* object_id_dev;
    long long object_id_host;
    double scale_mean[3];                                           /* config/category/<cat>.yaml: scale_mean */
    int regress_right;                                              /* the category regresses the right axis (:305-312) */
} CppfPoseTailItem;
int cppf_pose_tail_batch(int n_items, const CppfPoseTailItem* items_host, int F, const int* dims, int n_res, int out_dim, int tr_bins,
                         int rot_bins, int n_rots, const float* sphere32, const double* sphere64, int n_sphere, int sphere_sorted_by_y,
                         float thr, int64_t max_rot_pairs, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Back-vote filter.  Replaces `backvote_kernel` = CUDA `backvote` (models/voting.py:70-113),
 * launched at nocs/inference.py:216-228; always adaptive.
 *   out_offsets device f32[n_ppfs,3] zero-initialised by the caller (degenerate pairs are not
 *               written, as in the reference); may be NULL when only `mask` is wanted (degenerate
 *               pairs then get mask 0, as with a zero-initialised buffer)
 *   gt_center   device f32[3], tol = 3*res in the reference
 *   mask        device u8[n_ppfs] or NULL: any(out_offsets != 0) (nocs/inference.py:230)
 * ------------------------------------------------------------------------------------------- */
int cppf_backvote(const float* points, const float* outputs, float* out_offsets, const int32_t* point_idxs,
                  const float* corner, float res, int64_t n_ppfs, int n_rots, int gx, int gy, int gz,
                  const float* gt_center, float tol, uint8_t* mask, void* stream);
/* The same with (a) the dims optionally in a device record (shape_dev != NULL: gx, gy, gz ignored, see the `_dyn` section)
 * and (b) the workspace of the cppf_vote_argmax* call that produced gt_center (may be NULL): the vote leaves its (cos, sin)
 * rotation table there and the back-vote loads it instead of rebuilding it per workgroup.  Same results. */
int cppf_backvote_ws(const float* points, const float* outputs, float* out_offsets, const int32_t* point_idxs,
                     const float* corner, float res, int64_t n_ppfs, int n_rots, int gx, int gy, int gz,
                     const int32_t* shape_dev, const float* gt_center, float tol, uint8_t* mask,
                     const void* vote_workspace, void* stream);

/* Order-preserving compaction of the surviving pairs (point_idxs[mask], nocs/inference.py:231),
 * done on device.  surv: device i32[n] receives the indices i with mask[i] != 0 in increasing
 * order; count: device i32[1].  workspace >= cppf_compact_workspace_bytes(n). */
size_t cppf_compact_workspace_bytes(int64_t n);
int cppf_compact_mask(const uint8_t* mask, int64_t n, int32_t* surv, int32_t* count, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Shape-polymorphic (`_dyn`) variants: the instance shape lives in DEVICE memory.
 *
 * The reference runs one instance at a time and re-derives every size on the host (N after voxel de-duplication,
 * nocs/inference.py:140-142; grid dims, :194-195), so every instance has its own launch geometry.  A captured hipGraph
 * bakes by-value arguments in; these variants read `shape_dev` = device i32[4] {n_points, gx, gy, gz} instead, so ONE
 * captured chain serves every instance whose shape fits the launch's capacities.  Layout and results are those of the
 * by-value entry points for the same real shape, bit for bit: the kernels evaluate the same plan function on the device;
 * capacities only size allocations and launch geometry.
 *   cppf_vote_tiles           LDS tiles the vote needs for a grid (0: more than the tiled path serves) -- lets the caller
 *                             pick `many_tiles` (needed when any instance can need >= 4 tiles; costs the binning launch and the
 *                             room for the pair -> tile queues, see cppf_vote_workspace_bytes_dyn_pairs).  `many_tiles` is a tile
 *                             CAPACITY CLASS: 0 = up to 3 tiles (the fused kernel), 1 = up to 64 (any tiled grid), 4..64 = up to that
 *                             many (ABI 4: queues and reduce launch sized for them -- a posed NOCS object needs 9-12 tiles, the C5
 *                             grid 16: class 16 asks for a quarter of class 1's queues)
 *   cppf_vote_argmax_dyn      cppf_vote_argmax; grid_obj holds grid_capacity cells, the real grid f32[gx,gy,gz] occupies its
 *                             first gx*gy*gz cells; probs/points rows beyond n_points are never read.  A record that exceeds
 *                             a capacity (cells, n_points_cap, tiles) writes out_idx = -1, out_val = NaN and votes nothing.
 *   cppf_center_from_argmax_dyn, cppf_backvote_dyn   as their by-value forms, dims from the record
 *   cppf_knn_dyn, cppf_point_encoder_forward_dyn     n_points from n_dev (device i32[1], e.g. shape_dev); launches sized
 *                             for n_cap; rows >= n_points of nbrs / out are left untouched.  k <= n_points is the caller's duty.
 * ------------------------------------------------------------------------------------------- */
int cppf_vote_tiles(int gx, int gy, int gz);
int cppf_vote_tile_cells(void);   /* cells of one LDS tile: a launch serves grids of up to 3 (many_tiles = 1: 64; = n: n) times that */
/* Workspace of a *_dyn vote launch: the state block, the pair -> tile queues of the many-tile class (n_ppfs records of 12 B for
 * every tile of the class: sized for the worst case, every pair in every tile) and one partial tile per workgroup.
 * (ABI 1 had a second, smaller size that selected round 2's kernels; those are gone.) */
size_t cppf_vote_workspace_bytes_dyn_pairs(int many_tiles, int64_t n_ppfs);
/* The vote workspace keeps state between calls (queue counters and the plane of fixed-point wrap-arounds, see the note on
 * workspaces above): its first min(cppf_vote_workspace_init_bytes(), size) bytes must be ZERO before the first call on a
 * fresh allocation (one hipMemsetAsync); every call leaves them ready for the next one.  Calls on a workspace whose header
 * was never initialised report arg-max -1 / peak NaN -- every one of them, until the caller zeroes those bytes. */
size_t cppf_vote_workspace_init_bytes(void);
/* What a by-value vote launch will do for this problem (tests, tools): out int32[10] = {path, tiles, tx, ty, ntx, nty, halo_x,
 * halo_y, workgroups, fixed-point bits}; path 0: global fp32 atomics (> 64 tiles), 2: fused kernel (< 4 tiles), 3: binning +
 * queue-consuming kernels (>= 4 tiles); (1 was round 2's kernels: gone).  Host only, no device needed. */
int cppf_vote_plan_query(int64_t n_ppfs, int n_rots, int gx, int gy, int gz, int32_t* out);
int cppf_vote_argmax_dyn(const float* points, const float* outputs, const float* probs, const void* point_idxs,
                         int idx_is_i64, float* grid_obj, int64_t grid_capacity, const float* corner, float res,
                         int64_t n_points_cap, int64_t n_ppfs, int n_rots, const int32_t* shape_dev, int many_tiles,
                         int adaptive, int accumulate, long long* out_idx, float* out_val, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The votes of up to 8 objects -- the instances of a frame (nocs/inference.py:120 loops over them), each with its own cloud, pair
 * list, grid, results and vote workspace -- enqueued together.  Items on the tiled path (a grid of <= 64 LDS tiles; dims by value,
 * or from a device record when shape_dev != NULL) with n_rots <= 72 share ONE vote launch and ONE reduce launch: workgroups
 * [w_i, w_{i+1}) are item i's launch; an item whose grid needs >= 4 tiles (a posed object, a fine grid) first gets its own binning
 * launch.  Each object then runs on fewer, longer-lived workgroups -- cppf_vote_batch_workgroups(n, flags) each, n = the items that
 * share the launch: 256 / n (at least 64) unless CPPF_VOTE_WORKGROUPS(n) in `flags` says otherwise -- which divides the partial-tile
 * traffic per object (a workgroup zeroes, dumps and has read back its 113 KB tile whatever it deposits) without idling the rest of
 * the chip, and the launch prologue is paid once.  Every other item (n_rots > 72, an empty pair list, a grid beyond the tiled path)
 * gets the launches cppf_vote_argmax / cppf_vote_argmax_dyn would issue for it.  Per item the grid, arg-max and peak are those of
 * its own cppf_vote_argmax* call, bit for bit, whatever either call's width: the grid is the exact integer sum of the quantised
 * deposits and the fixed-point scale is that of a 64-wide launch at every width (both forms).  flags: as `accumulate` of
 * cppf_vote_argmax.  An item whose workspace is missing or shorter than its query refuses the whole batch (CPPF_EWORKSPACE)
 * before anything is launched: no item's grid, result or workspace state has been touched.  Replaces n launches of `ppf_kernel` (models/voting.py:8-66, nocs/inference.py:192-205) + np.argmax (:207-208). */
typedef struct CppfVoteItem {
    const float* points;      /* device f32[n_points,3] */
    const float* outputs;     /* device f32[n_ppfs,2] (mu, nu) */
    const float* probs;       /* device f32[n_points] or NULL (all ones) */
    const void* point_idxs;   /* device i32 / i64 [n_ppfs,2] */
    float* grid;              /* device f32[gx,gy,gz] (by value) or f32[grid_capacity] (shape_dev) */
    const float* corner;      /* device f32[3] */
    long long* out_idx;       /* device i64[1] */
    float* out_val;           /* device f32[1] */
    void* workspace;          /* cppf_vote_workspace_bytes(...) / cppf_vote_workspace_bytes_dyn_pairs(...), initialised as for the single calls */
    size_t workspace_bytes;
    const int32_t* shape_dev; /* NULL: gx, gy, gz, n_points by value; else device i32[4] {n_points, gx, gy, gz}, n_points = capacity */
    int64_t grid_capacity;    /* shape_dev only */
    int64_t n_points, n_ppfs;
    float res;
    int gx, gy, gz;
    int idx_is_i64;
    int many_tiles;           /* shape_dev only */
} CppfVoteItem;
int cppf_vote_batch_workgroups(int n_items, int flags);
int cppf_vote_argmax_batch(int n_items, const CppfVoteItem* items_host, int n_rots, int adaptive, int flags, void* stream);
int cppf_center_from_argmax_dyn(const long long* idx, const float* corner, double res, const int32_t* shape_dev, double* T64,
                                float* T32, const float* peak, double* idx_peak_f64, void* stream);
int cppf_backvote_dyn(const float* points, const float* outputs, float* out_offsets, const int32_t* point_idxs,
                      const float* corner, float res, int64_t n_ppfs, int n_rots, const int32_t* shape_dev,
                      const float* gt_center, float tol, uint8_t* mask, void* stream);
int cppf_knn_dyn(const float* pc, int n_cap, const int32_t* n_dev, int k, int32_t* nbrs, void* stream);
int cppf_point_encoder_forward_dyn(const float* pc, const float* nrm, const int32_t* nbrs, int n_cap, const int32_t* n_dev,
                                   int k, const float* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                                   int n_out, int n_glob, int num_layers, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* The point encoders of up to 8 instances -- models/model.py:47-57 per instance of the loop nocs/inference.py:120,180-181 -- in THREE
 * launches (search, convolution, GlobalInfoProp) instead of three per instance: what cppf_knn_dyn + cppf_point_encoder_forward_dyn
 * compute per cloud, bit for bit (ABI 4).  A cloud of 700-2000 points is that many wavefronts, a fraction of the chip; the members of
 * a chain fill it.  One-layer standard encoder only (train.py:34; anything else: CPPF_EUNSUPPORTED, call the per-cloud entry points).
 * Members may carry different weights (instances of different categories).  n_dev NULL: n_cap is the point count.
 * nbrs_ready != 0: `nbrs` already holds the member's neighbour sets (cppf_frame_cloud_dyn leaves them), no search for it. */
typedef struct CppfPointEncItem {
    const float* pc;          /* device f32[n_cap,3] */
    const float* nrm;         /* device f32[n_cap,3] */
    int32_t* nbrs;            /* device i32[n_cap,k] */
    const int32_t* n_dev;     /* device i32[1]: points in use, or NULL */
    const float* packed;      /* this member's encoder image (cppf_point_encoder_pack / _pack_device) */
    float* out;               /* device f32[n_cap, n_out + n_glob]; rows >= the point count are left untouched */
    void* workspace;          /* cppf_point_encoder_workspace_bytes(n_cap, n_out, n_glob, 1), the member's own */
    size_t workspace_bytes;
    int32_t n_cap;
    int32_t nbrs_ready;
} CppfPointEncItem;
int cppf_point_encoder_forward_batch(int n_items, const CppfPointEncItem* items_host, int k, const int32_t* hidden, int n_hidden,
                                     int rank, int n_nbr_feats, int n_out, int n_glob, int num_layers, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Orientation candidates.  Replaces `rot_voting_kernel` = CUDA `rot_voting`
 * (models/voting.py:115-148), launched at nocs/inference.py:265-275.
 *   preds_rot  device f32[n_ppfs]          outputs_up device f32[n_ppfs,n_rots,3], zero-initialised
 * ------------------------------------------------------------------------------------------- */
int cppf_rot_voting(const float* points, const float* preds_rot, float* outputs_up, const int32_t* point_idxs,
                    int64_t n_ppfs, int n_rots, void* stream);

/* Fused rot_voting + sphere-bin count (nocs/inference.py:265-284) without materialising the
 * [n,n_rots,3] candidates: for the pairs sel[0..min(*n_sel_dev, max_pairs)) (indices into the
 * pair arrays; sel == NULL -> pairs 0..), counts[j] += #(cand . sphere[j] > thr).
 *   preds_rot device f32, element i at preds_rot[i*rot_stride]
 *   sphere device f32[S,3]; counts device i32[S] zero-initialised by the caller
 *   n_sel_dev device i32[1] (number of valid entries of sel) or NULL -> n_sel_host
 *   sphere_sorted_by_y: +1 / -1 when the bins are unit vectors whose y column is sorted descending /
 *     ascending (the Fibonacci sphere of utils/util.py:102-118 is descending): enables the banded
 *     search (identical counts, ~30x less work); 0 = no assumption. */
int cppf_rot_sphere_count(const float* points, const float* preds_rot, int rot_stride, const int32_t* point_idxs,
                          const int32_t* sel, const int32_t* n_sel_dev, int64_t n_sel_host, int64_t max_pairs,
                          int n_rots, const float* sphere, int n_sphere, float thr, int sphere_sorted_by_y,
                          int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pair encoder.  Replaces PPFEncoder.forward_with_idx (models/model.py:117-137) incl. the PPF
 * construction (:118-129), the feature gather/concat (:132) and the ResLayer chain (:27-31).
 *   pc, nrm    device f32[N,3]    feat device f32[N,F]
 *   idxs       device i64[P,2] (idx_is_i64 != 0) or i32[P,2]
 *   packed     device f32[cppf_pair_mlp_packed_floats(...)], built by cppf_pair_mlp_pack()
 *   out        device f32[P,out_dim] logits
 * Supported on the MFMA path: dims = {2F+4, 32, 32, 16} with F = 40 and out_dim <= 144 (the only
 * architecture the reference trains, train.py:35); any other ResLayer stack runs on the generic
 * kernel (one pair per lane, at most 128 units per layer).  The MFMA path first projects every point
 * through the feat columns of layer 0 (N*128 floats in `workspace`), see csrc/pair_mlp.hip; it addresses with
 * 32-bit byte offsets and serves N < 2^23 points and P < 2^27 pairs per call (CPPF_EUNSUPPORTED beyond:
 * split the pair list).
 * ------------------------------------------------------------------------------------------- */
size_t cppf_pair_mlp_packed_floats(int F, const int* dims, int n_res, int out_dim);
/* device scratch for one call: the per-point layer-0 projection table of the MFMA path (N*128 floats),
 * 0 for the generic kernel */
size_t cppf_pair_mlp_workspace_bytes(int64_t N, int F, const int* dims, int n_res, int out_dim);
/* host-side packing: params/offs use the layout documented in oracle/cppf_oracle.c:orc_pair_mlp
 * (flat torch tensors + offset table: 6 per res layer {fc1.w, fc1.b, fc2.w, fc2.b, fc0.w|-1,
 * fc0.b|-1} then {final.w, final.b}); packed_host receives cppf_pair_mlp_packed_floats() floats. */
int cppf_pair_mlp_pack(const float* params, const int64_t* offs, int F, const int* dims, int n_res, int out_dim,
                       float* packed_host);
/* the same image built on the device from DEVICE parameters (`params` device f32, `offs` HOST): what a training
 * loop uses, where the weights change every step (train.py:92 optimizer.step) and a host pack would cost a device ->
 * host -> device round trip with a synchronisation.  MFMA path only (else CPPF_EUNSUPPORTED). */
int cppf_pair_mlp_pack_device(const float* params, const int64_t* offs, int F, const int* dims, int n_res, int out_dim,
                              float* packed_device, void* stream);
int cppf_pair_mlp_forward(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                          const float* packed, int64_t N, int F, const int* dims, int n_res, int64_t P,
                          int out_dim, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Pair encoder fused with the decode of nocs/inference.py:185-188 (+ :245-256 when heads != NULL):
 * softmax over the bins + inverse-CDF draw with caller-supplied uniforms (stand-in for
 * torch.multinomial; u < 0 selects the arg-max bin) + bin -> value.  Logits never leave the CU.
 *   u_tr  device f32[P,2]   -> outputs device f32[P,2] = (mu, nu)
 *   u_rot device f32[P,2]   -> heads   device f32[P,8] = {theta_up, theta_right, aux_up, aux_right,
 *                                                         sx, sy, sz, 0}    (both NULL to skip)
 * Requires the MFMA architecture above with tr_bins = 32, rot_bins = 36, out_dim = 141.
 * Arithmetic of the draw (restated in oracle/cppf_oracle.c:orc_sample_bin / orc_exp2w, bit for bit): weights
 * 2^(l log2e - max log2e) from a fixed degree-4 core (2.7e-6 relative, through the subnormals to zero for spreads beyond ~87),
 * summed in four consecutive segments of the bins, first bin whose running sum exceeds u * total.
 * Inputs of the pair-encoder entry points (clouds, normals, features, weights) must be finite: the file is built with
 * -fno-honor-nans, a NaN or infinity gives unspecified outputs (never a fault). */
int cppf_pair_mlp_decode(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                         const float* packed, int64_t N, int F, const int* dims, int n_res, int64_t P,
                         int out_dim, int tr_bins, int rot_bins, float vr0, float vr1, const float* u_tr,
                         const float* u_rot, float* outputs, float* heads, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same call for up to 8 pair lists in ONE launch -- the instances of a frame (nocs/inference.py:120 loops over them), each with
 * its own cloud, pair list, outputs, per-point workspace and weight image (the reference keeps one network per category, :79-90).
 * The lists get workgroups in proportion to their lengths; the ~9 us a launch spends before its first MFMA are paid once.
 * Results are those of n_items cppf_pair_mlp_decode calls, bit for bit.  All items with heads / u_rot or none.  A list with
 * n_pairs == 0 is CPPF_EINVAL here (the bf16 entry below skips it: the one difference between the two item contracts). */
typedef struct CppfPairMlpItem {
    const float* pc;        /* device f32[n_points,3] */
    const float* nrm;       /* device f32[n_points,3] */
    const float* feat;      /* device f32[n_points,F] */
    const void* idxs;       /* device i32 / i64 [n_pairs,2] */
    const float* packed;    /* device weight image (cppf_pair_mlp_pack) */
    const float* u_tr;      /* device f32[n_pairs,2] */
    const float* u_rot;     /* device f32[n_pairs,2] or NULL */
    float* outputs;         /* device f32[n_pairs,2] */
    float* heads;           /* device f32[n_pairs,8] or NULL */
    void* workspace;        /* device, cppf_pair_mlp_workspace_bytes(n_points, ...) */
    size_t workspace_bytes;
    int64_t n_points, n_pairs;
    float vr0, vr1;
    int idx_is_i64;
    /* cppf_pair_mlp_decode_sel_batch only (the first-pass entry ignores them): */
    const int32_t* sel;       /* device i32[>= max_sel]: the surviving pairs (cppf_compact_*'s output) */
    const int32_t* n_sel_dev; /* device i32[1]: how many */
    int64_t max_sel;          /* slots of the launch for this list (capacity; 0: skip the list) */
} CppfPairMlpItem;
int cppf_pair_mlp_decode_batch(int n_items, const CppfPairMlpItem* items_host, int F, const int* dims, int n_res, int out_dim,
                               int tr_bins, int rot_bins, void* stream);
/* The geometry that launch takes for lists of n_pairs[i] pairs (host arrays; no device work): *grid workgroups; *per_xcd > 0 = the
 * XCD-pinned mapping (1, 2, 4 or 8 lists within 10 % of each other: list i runs on XCDs [i per_xcd, (i + 1) per_xcd), so each
 * XCD's L2 holds ONE list's per-point table), 0 = contiguous workgroup ranges wg_begin[0..n_items] (optional output, may be NULL).
 * For callers that size batches and for tests that must know which mapping a launch exercised. */
int cppf_pair_mlp_batch_plan(int n_items, const int64_t* n_pairs, int* per_xcd, int* grid, int* wg_begin);
/* The second pass (cppf_pair_mlp_decode_sel, below) for up to 8 lists in one launch: list i's surviving pairs sel[0 .. min(*n_sel_dev,
 * max_sel)) get their heads rows; item.workspace must hold the per-point table its first pass left.  u_tr / outputs are not used. */
int cppf_pair_mlp_decode_sel_batch(int n_items, const CppfPairMlpItem* items_host, int F, const int* dims, int n_res, int out_dim,
                                   int tr_bins, int rot_bins, void* stream);

/* The second MLP pass of nocs/inference.py:236-256 -- ppf_encoder(..., idxs=point_idxs[mask]) followed by the decode of the
 * rotation bins, the sign logits and the log-scales -- on the surviving pairs only, without materialising point_idxs[mask]:
 * slot i < min(*n_sel_dev, max_sel) works on pair sel[i] (cppf_compact_mask's output) and writes heads[sel[i]]; u_rot is
 * indexed by ORIGINAL pair like heads.  Rows of pairs that are not selected are left untouched.  `workspace` must be the one
 * the preceding cppf_pair_mlp_decode call on the same (feat, packed) used: its per-point table is reused, not rebuilt.
 * The launch is sized for max_sel slots (a captured graph cannot know the count); surplus workgroups exit at once. */
int cppf_pair_mlp_decode_sel(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                             const float* packed, int64_t N, int F, const int* dims, int n_res, int64_t P, int out_dim,
                             int tr_bins, int rot_bins, const float* u_rot, const int32_t* sel, const int32_t* n_sel_dev,
                             int64_t max_sel, float* heads, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 pair encoder (opt-in; additive, ABI version unchanged).  The same kernel structure with the hidden layers on
 * v_mfma_f32_16x16x32_bf16 / _16x16x16_bf16: layer 0 (per-point tables, PPF inputs) stays fp32 exactly as above; after it every
 * product is bf16 x bf16 -- weights rounded to nearest even once by the packer, activations as they enter a layer -- and every
 * accumulation, bias and residual add is fp32 (the residual of layer 1 is the unrounded fp32 value).  Logits are fp32 and the decode
 * is the fp32 entry points' own arithmetic on them.  DESIGN.md "bf16 pair encoder" states the numerics; results are deterministic but
 * NOT those of the fp32 entry points.  Standard architecture only (dims = {84, 32, 32, 16}, F = 40, out_dim <= 144): anything else is
 * CPPF_EUNSUPPORTED -- there is no generic bf16 kernel and no fall-back to fp32.
 *   cppf_pair_mlp_bf16_packed_bytes   size of the weight image in BYTES (0: architecture not served)
 *   cppf_pair_mlp_bf16_pack / _pack_device   params / offs as cppf_pair_mlp_pack / cppf_pair_mlp_pack_device; the image holds bf16
 *                                     weights for every layer after layer 0, the layer-0 section and all biases in fp32
 *   cppf_pair_mlp_bf16_forward        logits f32[P,out_dim], any out_dim <= 144; workspace as cppf_pair_mlp_workspace_bytes()
 *   cppf_pair_mlp_bf16_decode_batch / _decode_sel_batch   cppf_pair_mlp_decode_batch / _decode_sel_batch with item.packed pointing at a
 *                                     bf16 image: up to 8 lists, the geometry of cppf_pair_mlp_batch_plan, CPPF_EUNSUPPORTED for other
 *                                     architectures and bin counts, CPPF_EWORKSPACE for a short workspace; a list with n_pairs == 0 is
 *                                     skipped; the sel pass reuses the table its first pass left.  One list is the batch of one.
 * ------------------------------------------------------------------------------------------- */
size_t cppf_pair_mlp_bf16_packed_bytes(int F, const int* dims, int n_res, int out_dim);
int cppf_pair_mlp_bf16_pack(const float* params, const int64_t* offs, int F, const int* dims, int n_res, int out_dim,
                            void* packed_host);
int cppf_pair_mlp_bf16_pack_device(const float* params, const int64_t* offs, int F, const int* dims, int n_res, int out_dim,
                                   void* packed_device, void* stream);
int cppf_pair_mlp_bf16_forward(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                               const void* packed, int64_t N, int F, const int* dims, int n_res, int64_t P, int out_dim,
                               float* out, void* workspace, size_t workspace_bytes, void* stream);
int cppf_pair_mlp_bf16_decode_batch(int n_items, const CppfPairMlpItem* items_host, int F, const int* dims, int n_res, int out_dim,
                                    int tr_bins, int rot_bins, void* stream);
int cppf_pair_mlp_bf16_decode_sel_batch(int n_items, const CppfPairMlpItem* items_host, int F, const int* dims, int n_res, int out_dim,
                                        int tr_bins, int rot_bins, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 point encoder (opt-in; additive, ABI version unchanged).  The SPRIN convolution of cppf_point_encoder_forward with layers
 * 2..5 of its per-neighbour kernel-MLP on v_mfma_f32_16x16x32_bf16: gather, rifeat and layer 1 (6 -> 32) stay fp32 exactly as above,
 * the four LayerNorms stay fp32 on the fp32 accumulators; the input of every later layer is bf(relu(LayerNorm(.))), its weights are
 * rounded to nearest even once by the packer, every product is bf16 x bf16 and every sum fp32 on the bias seed.  The last layer's
 * output is fp32 and not rounded; the rank contraction, the outnet, its LayerNorm and GlobalInfoProp are the fp32 entry points' own
 * arithmetic on it.  DESIGN.md 3.5a states the numerics; results are deterministic but NOT those of the fp32 entry points.
 * Serves what the fp32 kernel serves (hidden = {32,64,32,32}, rank 32, n_out 32, n_nbr_feats 2, k <= 64, any num_layers; the batch
 * entry one-layer encoders): anything else is CPPF_EUNSUPPORTED -- there is no generic bf16 kernel and no fall-back to fp32.
 *   cppf_point_encoder_bf16_packed_bytes   size of the weight image in BYTES (0: architecture not served)
 *   cppf_point_encoder_bf16_pack / _pack_device   `natural` as cppf_point_encoder_pack / _pack_device take it (host / device; the
 *                                     device form serves any num_layers); the image is the natural block verbatim followed per
 *                                     layer by 3 840 words: layer 1 and all bias / gamma / beta vectors in fp32, layers 2..5 in bf16
 *                                     (csrc/sprin_layout_bf16.h)
 *   cppf_point_encoder_bf16_forward / _forward_dyn / _forward_batch   arguments, workspace (cppf_point_encoder_workspace_bytes) and
 *                                     return codes of cppf_point_encoder_forward / _forward_dyn / _forward_batch, with `packed`
 *                                     (CppfPointEncItem.packed) pointing at a bf16 image: CPPF_EINVAL for null pointers,
 *                                     CPPF_EUNSUPPORTED for another architecture or k > 64, CPPF_EWORKSPACE for a short workspace;
 *                                     n_points == 0 is a no-op
 * ------------------------------------------------------------------------------------------- */
size_t cppf_point_encoder_bf16_packed_bytes(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                            int num_layers);
int cppf_point_encoder_bf16_pack(const float* natural /*host*/, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                                 int n_out, int n_glob, int num_layers, void* packed_host);
int cppf_point_encoder_bf16_pack_device(const float* natural /*device*/, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                                        int n_out, int n_glob, int num_layers, void* packed_device, void* stream);
int cppf_point_encoder_bf16_forward(const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k, const void* packed,
                                    const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                    int num_layers, float* out, void* workspace, size_t workspace_bytes, void* stream);
int cppf_point_encoder_bf16_forward_dyn(const float* pc, const float* nrm, const int32_t* nbrs, int n_cap, const int32_t* n_dev, int k,
                                        const void* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                        int n_glob, int num_layers, float* out, void* workspace, size_t workspace_bytes, void* stream);
int cppf_point_encoder_bf16_forward_batch(int n_items, const CppfPointEncItem* items_host, int k, const int32_t* hidden, int n_hidden,
                                          int rank, int n_nbr_feats, int n_out, int n_glob, int num_layers, void* stream);

#ifdef CPPF_DEBUG_ENTRY
/* Profiling aid, compiled only with -DCPPF_DEBUG_ENTRY (not in the shipped library): the PPF + gather + MFMA chain of the
 * standard architecture with no epilogue (isolates the matrix pipeline when reading rocprof counters).
 * scratch: >= 4 bytes of device memory (never written in practice). */
int cppf_debug_mlp_chain_only(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                              const float* packed, int64_t N, int64_t P, float* scratch, void* workspace,
                              size_t workspace_bytes, void* stream);
#endif

/* Decode from logits already in memory (generic architectures / bin counts). */
int cppf_decode_center(const float* logits, int64_t P, int ld, int tr_bins, float vr0, float vr1,
                       const float* u_tr, float* outputs, void* stream);
int cppf_decode_rot(const float* logits, int64_t P, int ld, int out_dim, int tr_bins, int rot_bins,
                    const float* u_rot, float* heads, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reductions of the pose tail.
 *  cppf_axis_sign: nocs/inference.py:287-301.  For pairs sel[0..*n_sel_dev): flip n_a to agree with
 *    ab, target = (n . best_dir > 0), sums of BCEWithLogits(aux, target) and (aux, 1-target).
 *    aux element i at aux[i*aux_stride]; best_dir device f64[3]; out device f64[3] =
 *    {up_loss_sum, down_loss_sum, n}.  The caller compares the two means.
 *  cppf_scale_sum: nocs/inference.py:335.  out device f64[4] = {sum sx, sum sy, sum sz, n} over the
 *    selected pairs; the caller finishes exp(mean)*scale_mean*2.
 *  Both are two-kernel deterministic reductions (fixed order), workspace >= cppf_reduce_workspace_bytes().
 * ------------------------------------------------------------------------------------------- */
size_t cppf_reduce_workspace_bytes(void);
int cppf_axis_sign(const float* pc, const float* nrm, const int32_t* point_idxs, const int32_t* sel,
                   const int32_t* n_sel_dev, int64_t n_sel_host, const float* aux, int aux_stride,
                   const double* best_dir, double* out, void* workspace, size_t workspace_bytes, void* stream);
int cppf_scale_sum(const float* scale_logits, int stride, const int32_t* sel, const int32_t* n_sel_dev,
                   int64_t n_sel_host, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* cppf_scale_exp_sum: the same sums of expf(logit) -- the mean of exp of nocs/zero_shot.ipynb cell 11
 *   (np.mean(np.exp(preds_scale) * scale_mean * 2, 0)); out = {sum e^sx, sum e^sy, sum e^sz, n}. */
int cppf_scale_exp_sum(const float* scale_logits, int stride, const int32_t* sel, const int32_t* n_sel_dev,
                       int64_t n_sel_host, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The pose tail in six launches (nocs/inference.py:209-303,335 after the centre vote).  The entry points above map one
 * to one onto the reference's steps; these fuse neighbours whose only separation was a launch boundary, with identical
 * results (the integer outputs bit for bit; the fp64 sums of cppf_pose_sums within 1e-12 relative of the two-kernel forms:
 * other order of the final partial sum).
 *  cppf_pose_tail_begin: cppf_center_from_argmax(_dyn) (shape_dev non-null: dims from the record) that first zeroes
 *    zero_bytes (multiple of 16, 16-byte aligned) at zero_ptr: the bin counts, chunk counts, ticket and result record of
 *    the launches below.  T64 / idx_peak_f64 may lie inside the region.
 *  cppf_backvote_count: cppf_backvote_ws writing the mask only, plus chunk_counts[i] += survivors among pairs
 *    [1024 i, 1024 i + 1024) (int32[(n_ppfs + 1023) / 1024], zero on entry).
 *  cppf_compact_scatter: cppf_compact_mask given those counts (no counting pass, no scan launch).  n <= 8192 * 1024
 *    pairs (CPPF_EUNSUPPORTED beyond: use cppf_compact_mask).
 *  cppf_rot_sphere_count_dirs: cppf_rot_sphere_count for n_dirs angle columns in one launch: direction j reads
 *    preds_rot[p * rot_stride + j * rot_dir_step] and adds to counts[j * counts_dir_step + bin].
 *  cppf_pose_sums: np.argmax of each direction's counts and best_dir = sphere64[argmax] (cppf_counts_argmax_select),
 *    the sign sums of each direction (cppf_axis_sign; aux of direction j at aux[p * aux_stride + j]) and the scale sums
 *    (cppf_scale_sum; scale_logits may be null) in one launch.  best_idx i64[n_dirs] (may be null), best_dir f64[n_dirs][3],
 *    sign f64[n_dirs][3], scale_out f64[4]; n_dirs <= 2; workspace >= cppf_pose_sums_workspace_bytes(); ticket: one
 *    device uint32, zero before the first call and left at zero.
 * ------------------------------------------------------------------------------------------- */
int cppf_pose_tail_begin(const long long* idx, const float* corner, double res, int gy, int gz, const int32_t* shape_dev,
                         double* T64, float* T32, const float* peak, double* idx_peak_f64, void* zero_ptr,
                         size_t zero_bytes, void* stream);
int cppf_backvote_count(const float* points, const float* outputs, const int32_t* point_idxs, const float* corner,
                        float res, int64_t n_ppfs, int n_rots, int gx, int gy, int gz, const int32_t* shape_dev,
                        const float* gt_center, float tol, uint8_t* mask, int32_t* chunk_counts,
                        const void* vote_workspace, void* stream);
/* cppf_backvote_count reading the pair list as int64 (the caller's np.random.randint array, nocs/inference.py:177) and leaving
 * its int32 copy in idx32_out (int32[n_ppfs][2], may be null) for the launches that follow. */
int cppf_backvote_count64(const float* points, const float* outputs, const long long* point_idxs64, int32_t* idx32_out,
                          const float* corner, float res, int64_t n_ppfs, int n_rots, int gx, int gy, int gz,
                          const int32_t* shape_dev, const float* gt_center, float tol, uint8_t* mask, int32_t* chunk_counts,
                          const void* vote_workspace, void* stream);
int cppf_compact_scatter(const uint8_t* mask, int64_t n, const int32_t* chunk_counts, int32_t* surv, int32_t* count,
                         void* stream);
int cppf_rot_sphere_count_dirs(const float* points, const float* preds_rot, int rot_stride, int rot_dir_step, int n_dirs,
                               const int32_t* point_idxs, const int32_t* sel, const int32_t* n_sel_dev,
                               int64_t n_sel_host, int64_t max_pairs, int n_rots, const float* sphere, int n_sphere,
                               float thr, int sphere_sorted_by_y, int32_t* counts, int counts_dir_step, void* stream);
/* cppf_rot_sphere_count_dirs on a caller-chosen subsample: slot k < min(n_order, max_pairs) takes the survivor at position
 * order[k] of `sel` (positions outside [0, *n_sel_dev) contribute nothing).  The reference draws its 10 000 pairs by shuffling
 * the survivors (nocs/inference.py:277-280: idxs = arange(P'); np.random.shuffle(idxs); idxs[:10000]); passing that shuffled
 * prefix as `order` (device int32[n_order]) reproduces its subsample exactly.  Without it the first max_pairs survivors in
 * pair order are taken -- the same distribution, since pairs are i.i.d. */
int cppf_rot_sphere_count_dirs_order(const float* points, const float* preds_rot, int rot_stride, int rot_dir_step, int n_dirs,
                                     const int32_t* point_idxs, const int32_t* sel, const int32_t* n_sel_dev,
                                     int64_t n_sel_host, const int32_t* order, int64_t n_order, int64_t max_pairs, int n_rots,
                                     const float* sphere, int n_sphere, float thr, int sphere_sorted_by_y, int32_t* counts,
                                     int counts_dir_step, void* stream);
size_t cppf_pose_sums_workspace_bytes(void);
int cppf_pose_sums(const float* pc, const float* nrm, const int32_t* point_idxs, const int32_t* sel,
                   const int32_t* n_sel_dev, int64_t n_sel_host, const float* aux, int aux_stride, int n_dirs,
                   const int32_t* counts, int n_sphere, int counts_dir_step, const double* sphere64,
                   const float* scale_logits, int scale_stride, long long* best_idx, double* best_dir, double* sign,
                   double* scale_out, void* workspace, size_t workspace_bytes, unsigned* ticket, void* stream);

/* nocs/inference.py:194-195 on device: corner = min(pc), dims = int32((max-min)/res)+1.
 * corner device f32[3], dims device i32[3]. */
int cppf_grid_setup(const float* pc, int64_t N, float res, float* corner, int32_t* dims, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SPRIN point encoder: produces the per-point `feat` the pair MLP gathers.
 * Replaces models/model.py:36-78 `PointEncoder.forward(pc, pc_normal, dist)` / `forward_nbrs(...)` with
 * models/sprin.py:40-107 (rifeat, conv_kernel, SparseSO3Conv, GlobalInfoProp), called at
 * nocs/inference.py:180-181 and train.py:62-64.
 *
 * cppf_knn: the neighbour sets of `torch.topk(dist, k, largest=False)` (models/model.py:47).
 *   dist != NULL: device f32[N,N], keys are dist[i][j] (the matrix the reference passes in);
 *   dist == NULL: keys are exact squared distances from pc (device f32[N,3]) -- no N x N matrix.
 *   nbrs: device i32[N,k], each row the k smallest keys (ties -> lower index) in ascending index order.
 *   One wavefront per query, keys streamed twice: the k-th smallest of the 64 per-lane minima bounds the
 *   answer, the ~3k keys below that bound are compacted into LDS and an exact 32-step bisection runs on them.
 *
 * cppf_point_encoder_forward: forward_nbrs.  pc, nrm device f32[N,3]; nbrs device i32[N,k], k <= 64;
 *   out device f32[N, n_out+n_glob].  `packed` device f32 = the image cppf_point_encoder_pack() builds on the host
 *   from the parameters in NATURAL order, which is per layer
 *     for each hidden width h_i (in_i = 6, then h_{i-1}):  W[h_i][in_i], b[h_i], ln_weight[h_i], ln_bias[h_i]
 *     Wk[rank][h_last], bk[rank]                      (spconvs.l.kernel.*)
 *     Wo_t[rank*n_in][n_out] = outnet.weight TRANSPOSED, bo[n_out], ln_weight[n_out], ln_bias[n_out]
 *     Wa[n_glob][n_out], ba[n_glob]                   (aggrs.l.linear)
 *   with n_in = n_nbr_feats (must be 2) for layer 0 and n_out+n_glob after it.  The image is that block followed,
 *   for the supported shape, by a lane-ordered copy of each layer's kernel-MLP weights for the MFMA kernel.
 *   Device kernel exists for hidden = {32,64,32,32}, rank = 32, n_out = 32, n_glob <= 32 (the
 *   configuration of train.py:34 / nocs/inference.py:82); anything else returns CPPF_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
int cppf_knn(const float* pc, const float* dist, int n_points, int k, int32_t* nbrs, void* stream);
size_t cppf_point_encoder_packed_floats(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                        int n_glob, int num_layers);
int cppf_point_encoder_pack(const float* natural /*host*/, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                            int n_out, int n_glob, int num_layers, float* packed_out /*host, packed_floats() long*/);
size_t cppf_point_encoder_workspace_bytes(int n_points, int n_out, int n_glob, int num_layers);
int cppf_point_encoder_forward(const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k,
                               const float* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                               int n_out, int n_glob, int num_layers, float* out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the pair encoder.  The reference has no backward code: train.py:91
 * calls loss.backward() and torch autograd differentiates models/model.py:117-137; this entry point returns
 * the same gradients for ppffcs = {84,32,32,16} (train.py:35), F = 40, any out_dim (else CPPF_EUNSUPPORTED).
 *   params       device f32, the parameters in torch layout, flat: per res layer fc1.weight, fc1.bias,
 *                fc2.weight, fc2.bias, [fc0.weight, fc0.bias], then final.weight, final.bias
 *   offs         HOST i64[6*n_res+2]: offset of each of those tensors in `params` (-1 for an absent fc0)
 *   grad_out     device f32[n_pairs, out_dim]  (dL/dlogits)
 *   grad_params  device f32, same layout as `params`, OVERWRITTEN
 *   grad_feat    device f32[n_points, F], ACCUMULATED (+=; zero it first for a plain gradient)
 * Formulation (cppf_amd/csrc/pair_mlp_bwd.hip): one workgroup of four wavefronts per tile of 64 pairs recomputes the
 * forward and back-propagates on the fp32 matrix cores; weight-gradient tiles accumulate in registers over all the
 * workgroup's pairs and are written once to one of at most CPPF_BWD_MAX_PARTS partial gradients in the workspace
 * (tiles dealt evenly), which are then added in a fixed two-level order.  Everything that touches the 2 x 40 feature
 * columns of layer 0 is done per POINT: each pair emits one 64-float row, the 2*n_pairs (point, entry) keys are radix
 * sorted (stable), every point adds its rows in pair order per role, and d(feat) and the feature columns of the two
 * layer-0 weight gradients are products of those sums.  No atomics anywhere: every result is deterministic
 * (oracle/backward_oracle.c restates the order).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_BWD_MAX_PARTS 512
size_t cppf_pair_mlp_backward_workspace_bytes(int64_t n_pairs, int64_t n_points, int F, const int* dims, int n_res,
                                              int out_dim);
int cppf_pair_mlp_backward(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                           const float* params, const int64_t* offs, int64_t n_points, int F, const int* dims, int n_res,
                           int64_t n_pairs, int out_dim, const float* grad_out, float* grad_params, float* grad_feat,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the point encoder: gradients of the parameters of the one-layer standard encoder (train.py:34: hidden
 * {32,64,32,32}, rank 32, 2 neighbour features, n_out 32, n_glob 8, k <= 64; anything else CPPF_EUNSUPPORTED).  The
 * reference has no backward code -- train.py:91 differentiates models/model.py:46-61 + models/sprin.py:40-107 with
 * autograd; points and normals carry no gradient there (train.py:58-60).
 *   packed       device f32: natural parameters + forward image, as cppf_point_encoder_forward takes them
 *   out_fwd      device f32[n_points, 40]: the forward output for the same inputs (the pooled maxima are read from it)
 *   contraction  device f32[n_points, 64] kept by cppf_point_encoder_forward_train, or NULL: the backward then recomputes
 *                it (one more forward pass of the kernel-MLP per point); the result is the same bit for bit
 *   grad_out     device f32[n_points, 40]
 *   grad_packed  device f32[9 256]: d/d(natural parameters) in the natural layout (outnet weight transposed), OVERWRITTEN
 * cppf_point_encoder_pack_device builds `packed` from natural parameters that already live on the device (training).
 * One wavefront per point, at most CPPF_SPRIN_BWD_MAX_PARTS partial gradients added in a fixed two-level order: the
 * result is deterministic (oracle/sprin_bwd_oracle.c restates the order).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_SPRIN_BWD_MAX_PARTS 1024
size_t cppf_point_encoder_backward_workspace_bytes(int n_points);
int cppf_point_encoder_pack_device(const float* natural, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                   int n_glob, int num_layers, float* packed, void* stream);
int cppf_point_encoder_backward(const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k, const float* packed,
                                const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                int num_layers, const float* out_fwd, const float* contraction, const float* grad_out,
                                float* grad_packed, void* workspace, size_t workspace_bytes, void* stream);
/* cppf_point_encoder_forward that also keeps the per-point contraction (einsum of models/sprin.py:99) for the backward */
int cppf_point_encoder_forward_train(const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k,
                                     const float* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats,
                                     int n_out, int n_glob, int num_layers, float* out, float* contraction_out, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pre-processing in front of the path.  Both replace third-party host calls whose
 * results are not fully specified, so parity with the reference is unpinned; the definitions are in
 * oracle/preproc_oracle.c.
 *  cppf_voxel_dedupe     the role of ME.utils.sparse_quantize(pc, return_index=True, quantization_size=res)[1]
 *                        (nocs/inference.py:140): keep_idx device i32[n_points] receives, in ascending order, the lowest
 *                        index of every occupied voxel floor(p / res) (fp64 divide); count device i32[1] = how many.
 *                        RANGE: per axis v = floor((double)p / res); a point is in range iff it is finite and
 *                        -2^20 <= v < 2^20 on all three axes (the voxel key holds 21 bits per axis).  If ANY point is out of
 *                        range the call writes count[0] = -1 and keep_idx is unspecified: distinct voxels are never merged,
 *                        the cloud is refused (a cloud left in millimetres with a metre-sized res, a NaN).  The refusal is
 *                        decided on the stream; the call does not synchronise.
 *  cppf_estimate_normals open3d estimate_normals(KDTreeSearchParamKNN(knn)) (utils/util.py:61-65): nbrs device
 *                        i32[n_points, k] (cppf_knn output: the point itself is a neighbour); normals device
 *                        f32[n_points, 3] = unit eigenvector of the smallest eigenvalue of the neighbours' covariance
 *                        (fp64 cumulants, 8 Jacobi sweeps), sign: component of largest magnitude positive.
 *  cppf_backproject      utils/util.py:598-631 `backproject(depth, intrinsics, instance_mask)` (nocs/inference.py:131): the
 *                        pixels with mask != 0 and depth > 0, in row-major order, back-projected through inv(intrinsics) in
 *                        fp64: pts device f64[H*W,3] (x and y negated like the reference's return value), pix device
 *                        i32[H*W] = v*W + u of each point (the reference's `idxs`), count device i32[1].  depth: device
 *                        u16[H,W] (depth_is_u16 != 0; NOCS depth PNGs) or f32[H,W]; mask device u8[H,W]; kinv_host: HOST
 *                        f64[9], row-major inverse of the 3x3 intrinsics.
 * ------------------------------------------------------------------------------------------- */
/* The whole per-instance pre-processing of nocs/inference.py:131-142 + the grid set-up of :194-195 as ONE count-driven stage for
 * captured, shape-polymorphic chains: no size visits the host.  A frame's depth image and a LABEL image (bit `label_bit` of pixel p
 * set <=> p belongs to the instance: up to 8 / 16 / 32 possibly overlapping instance masks in one upload) stay on the device;
 * the stage back-projects the instance's valid pixels (cppf_backproject's arithmetic), divides by `divisor` (1000: millimetres,
 * :132), flips x and y (:136-137), de-duplicates per voxel of edge `res` (cppf_voxel_dedupe's definition and RANGE, :140-141), writes the cloud
 * to pc_out f32[n_cap,3], its PCA normals over knn_k neighbours (cppf_knn + cppf_estimate_normals, :142) to nrm_out f32[n_cap,3], the
 * grid corner to corner_out f32[3] and the instance's shape record to shape_out i32[4] = {N, gx, gy, gz} -- what the *_dyn entry
 * points read.  N = 0 (and a 1x1x1 grid) when fewer than k_min points are left: the reference skips such instances (:121-123);
 * the *_dyn vote then reports arg-max -1.  A member with a point outside cppf_voxel_dedupe's RANGE (a voxel index beyond +-2^20, a
 * non-finite depth) reports N = 0 in the same way -- refused, not merged -- and leaves the other members of a batch untouched.  n_cap >= the number of set label pixels (the caller counts them on the host) bounds
 * every buffer; rows >= N of pc_out / nrm_out are left untouched.  nbrs_out (may be NULL): device i32[n_cap, knn_k] that receives the
 * neighbour sets the normals were fitted on -- cppf_knn's output, which a point encoder with the same k can reuse instead of
 * searching again (nocs/inference.py:180 computes the same cdist + topk).  Results equal the four single calls on the same inputs, bit for
 * bit.  Both entry points are cppf_frame_cloud_dyn_batch (below) for one member without pair draws, so like it they return
 * CPPF_EUNSUPPORTED for a frame of more than 8 388 608 pixels (8 192 compaction chunks of 1 024).  cppf_mod_pairs_dyn: idx[i] <- idx[i] mod N for pairs drawn as full-range non-negative integers before N was known (:177). */
size_t cppf_frame_cloud_workspace_bytes(int H, int W, int n_cap, int knn_k);
int cppf_frame_cloud_dyn(const void* depth, int depth_is_u16, const void* labels, int label_bytes, int label_bit, int H, int W,
                         const double* kinv_host, double divisor, double res, int knn_k, int k_min, int n_cap, float* pc_out,
                         float* nrm_out, float* corner_out, int32_t* shape_out, int32_t* nbrs_out, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The same with the label bit read from device memory at run time (*label_bit_dev, taken modulo the label width): ONE captured launch
 * serves whichever instance of a frame is handed to it -- a video whose instances change order, number or mask size replays the
 * graphs it has (cppf_amd.frames.FrameRunner keeps them per (category, capacity) and writes {bit, seed} per frame). */
int cppf_frame_cloud_dyn_bit(const void* depth, int depth_is_u16, const void* labels, int label_bytes, const int32_t* label_bit_dev, int H,
                             int W, const double* kinv_host, double divisor, double res, int knn_k, int k_min, int n_cap, float* pc_out,
                             float* nrm_out, float* corner_out, int32_t* shape_out, int32_t* nbrs_out, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The frame stage of up to 8 instances of ONE frame (nocs/inference.py:120 loops over them) in EIGHT launches, their pair lists and
 * bin uniforms included (the key read from *seed_dev): per instance the results of the four single calls above (cppf_backproject,
 * cppf_voxel_dedupe, cppf_knn, cppf_estimate_normals) and the draws of cppf_sample_pairs, bit for bit (ABI 4).  A frame's chain is
 * launch-bound -- a hipGraph launch costs the host per kernel node -- so a launch serves every member (blockIdx.y), the mask kernels
 * count their own chunks (no count + scan launches), the first one clears the voxel table, the normals launch also sets up the grid
 * and draws the pairs.  Every member has its own capacity, resolution, k, workspace (cppf_frame_cloud_workspace_bytes) and outputs. */
typedef struct CppfFrameCloudItem {
    const int32_t* label_bit_dev;          /* device i32: the member's bit of the label image (taken modulo the label width) */
    const unsigned long long* seed_dev;    /* device u64: Philox key of its pair / uniform draws (n_pairs > 0) */
    float* pc_out;                         /* device f32[n_cap,3] */
    float* nrm_out;                        /* device f32[n_cap,3] */
    float* corner_out;                     /* device f32[3] */
    int32_t* shape_out;                    /* device i32[4] {N (0: fewer than k_min points, or a point out of the voxel range), gx, gy, gz} */
    int32_t* nbrs_out;                     /* device i32[n_cap,knn_k] or NULL (kept in the workspace) */
    void* idx;                             /* device i64[n_pairs,2] (idx_is_i64) or i32[n_pairs,2] */
    float* u_tr;                           /* device f32[n_pairs,2] or NULL */
    float* u_rot;                          /* device f32[n_pairs,2] or NULL */
    void* workspace;
    size_t workspace_bytes;
    double res;
    int64_t n_pairs;                       /* 0: no draws */
    int32_t knn_k, k_min, n_cap, idx_is_i64;
} CppfFrameCloudItem;
int cppf_frame_cloud_dyn_batch(int n_items, const CppfFrameCloudItem* items_host, const void* depth, int depth_is_u16, const void* labels,
                               int label_bytes, int H, int W, const double* kinv_host, double divisor, void* stream);
/* Pair list and bin uniforms drawn on the device -- the reference draws the pairs with np.random.randint(0, N, (P, 2)) on the host
 * (nocs/inference.py:177: 8 MB per instance at C2 over PCIe) and the bins with torch.multinomial (:186,250,254).  idx device
 * i64[n_pairs,2] uniform over [0, N); u_tr / u_rot device f32[n_pairs,2] uniform over [0, 1) (either may be NULL).  N = n_points, or
 * *n_dev (device i32) when n_dev != NULL.  Philox-4x32-10 keyed by `seed`, counter = pair index: the draw of a pair is a function of
 * (seed, pair index) alone; seed_dev != NULL: the seed is read from device memory instead (a captured launch replayed with a new seed
 * per frame).  With N = 0 every index is 0.  Same distributions as the reference's generators, not the same numbers (parity tests pass arrays). */
int cppf_sample_pairs(long long* idx, float* u_tr, float* u_rot, int64_t n_pairs, int64_t n_points, const int32_t* n_dev,
                      unsigned long long seed, const unsigned long long* seed_dev, void* stream);
/* Host helper (no device): the grid of nocs/inference.py:194-195 for a HOST cloud f32[n_points,3]: corners_host f32[6] = {min xyz, max xyz},
 * dims_host i32[3] = int32((max - min) / res) + 1 with the quotient in fp32.  A cloud with a NaN / inf coordinate anywhere returns
 * CPPF_ENONFINITE (numpy's min / max would propagate it into the dims: the reference fails at np.zeros(grid_res), :196). */
int cppf_host_grid_shape(const float* pc_host, int64_t n_points, float res, float* corners_host, int32_t* dims_host);
int cppf_mod_pairs_dyn(long long* idx, int64_t n_pairs, const int32_t* n_dev, void* stream);
/* The head of a captured chain for objects that are ALREADY on the device ("inputs already resident on device"): for up
 * to 8 objects, ONE launch copies each object's cloud, normals and (optional) per-point features from wherever the caller keeps them
 * into the chain's own buffers, sets up its vote grid (nocs/inference.py:194-195: corner = min(pc), dims = int32((max - min) / res) + 1,
 * as cppf_grid_setup) and draws its pair list and bin uniforms (:177,186,250: as cppf_sample_pairs, bit for bit, with seed = desc.seed).
 * What changes from one replay to the next -- where the object lives, how many points it has, its seed, its id -- is read from a
 * DESCRIPTOR in device memory (the caller rewrites the descriptors with one small copy before each replay); what does not -- the
 * chain's buffers -- travels by value, so the launch is capturable in a hipGraph.  The reference's counterpart is the host side of the
 * instance loop, nocs/inference.py:120-142,177,194-196 (numpy arrays uploaded per instance). */
typedef struct CppfStageDesc {          /* DEVICE memory, 48 bytes, one per object of the chain */
    const float* pc_src;                /* device f32[n_points,3] */
    const float* nrm_src;               /* device f32[n_points,3] */
    const float* feat_src;              /* device f32[n_points,F] or NULL (features come from a point encoder in the chain) */
    long long n_points;                 /* <= the item's n_cap (the caller checks) */
    unsigned long long seed;            /* Philox key of the pair / uniform draws */
    long long object_id;                /* copied into the pose record (CppfPoseTailItem.object_id_dev may point here) */
} CppfStageDesc;
typedef struct CppfStageItem {          /* host memory, by value at launch: the chain's buffers */
    const CppfStageDesc* desc;          /* device */
    float* pc; float* nrm; float* feat; /* device f32[n_cap,3], f32[n_cap,3], f32[n_cap,F] (feat NULL: not copied) */
    float* corner;                      /* device f32[3] */
    int32_t* shape;                     /* device i32[4] <- {n_points, gx, gy, gz}, or NULL (a static-shape pipeline: only `corner` is written) */
    void* idx;                          /* device i64[n_pairs,2] (idx_is_i64) or i32[n_pairs,2], or NULL (no draw) */
    float* u_tr; float* u_rot;          /* device f32[n_pairs,2] each; either may be NULL */
    int64_t n_pairs, n_cap;
    int F;
    float res;
    int idx_is_i64;                     /* 1: the reference's int64 pair list (nocs/inference.py:177); 0: int32 -- half the index bytes for
                                         * every kernel of the chain that streams the list (the values are < n_points < 2^31 either way) */
} CppfStageItem;
int cppf_stage_batch(int n_items, const CppfStageItem* items_host, void* stream);
/* n_words 64-bit words from src to dst by a KERNEL of `stream` (8-byte aligned; either side may be pinned host memory, which the device
 * reads / writes in place).  For the few hundred bytes a batch driver moves per chain -- descriptors in, records out: a copy engine's
 * queue is shared between streams and in order, so such copies can wait behind another stream's unrelated transfer. */
int cppf_copy_words(void* dst, const void* src, int64_t n_words, void* stream);
/* row r of dst (n_words 64-bit words each) <- the words at src_host[r] (a HOST array of up to 32 device pointers, 8-byte aligned), one
 * launch: the result records of a chain's members into one array instead of one small copy per member (ABI 4) */
int cppf_gather_words(int n_rows, const void* const* src_host, int64_t n_words, void* dst, void* stream);
size_t cppf_backproject_workspace_bytes(int H, int W);
int cppf_backproject(const void* depth, int depth_is_u16, const uint8_t* mask, int H, int W, const double* kinv_host,
                     double* pts, int32_t* pix, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_voxel_dedupe_workspace_bytes(int64_t n_points);
int cppf_voxel_dedupe(const float* pc, int64_t n_points, double res, int32_t* keep_idx, int32_t* count, void* workspace,
                      size_t workspace_bytes, void* stream);
int cppf_estimate_normals(const float* pc, const int32_t* nbrs, int64_t n_points, int k, float* normals, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Zero-shot scene path (nocs/zero_shot.ipynb cells 6, 9, 11: one depth frame with no instance masks -> proposals, point masks,
 * poses; csrc/scene.hip).  The Python side is cppf_amd/zero_shot.py; tests/zero_shot_ref.py restates every result bit for bit.
 *
 * cppf_pair_filter_distinct (cell 6): keep[p] = 0 for the "indistinguishable" pairs, |n1.n2| > 0.9 & |ab.n1| < 0.1 & |ab.n2| < 0.1
 *   with ab = (a - b) / (||a - b|| + 1e-7), float32 like numpy; 1 otherwise.  point_idxs device i32 / i64 [n_pairs,2]; a pair with an
 *   endpoint outside [0, n_points) gets 0.  keep device u8[n_pairs]; the ordered list of the kept pairs is cppf_compact_mask's.
 *
 * cppf_gaussian_filter3d (cell 9, scipy.ndimage.gaussian_filter(grid, sigma), mode 'reflect'): bit for bit scipy's result for
 *   float32 grids.  One pass per axis (0, 1, 2); each output is w[r] x[c] + sum_{d = r..1} (x[c-d] + x[c+d]) w[r-d] in fp64 from the
 *   float32 input, rounded to float32 per pass; 'reflect' boundaries (= np.pad 'symmetric', repeated for axes shorter than r) for
 *   any dims >= 1.  weights: HOST f64[2 radius + 1], symmetric (scipy's _gaussian_kernel1d; radius = int(truncate sigma + 0.5) <= 32).
 *   grid, out device f32[gx,gy,gz], distinct; gx gy gz < 2^30; workspace >= cppf_gaussian_filter3d_workspace_bytes().
 *
 * cppf_scene_proposals (cell 9, the whole proposal loop, on the device: graph-capturable, no host round trip): smooths `grid` (the
 *   raw scene vote) as cppf_gaussian_filter3d does, writes that smoothed grid to smoothed_out when it is not NULL (the caller's copy
 *   is never suppressed), then loops:
 *     loc = first arg-max (C order); lll = max(0, loc - margin), rrr = min(dim - 1, loc + margin);
 *     diff = smoothed[loc] - (the mean of the notebook's 12 float32 edge means, slices half-open lll:rrr, np.mean's order);
 *     diff > thresh: record (loc, smoothed[loc], diff), the first recorded diff is max_val;
 *     stop when diff < thresh or diff < 0.7 max_val; else zero smoothed[lll:rrr, lll:rrr, lll:rrr] and repeat.
 *   Outputs (device): loc i32[max_proposals,3], value f32[max_proposals], diff f32[max_proposals], count i32[1].
 *   Defined where the notebook is not:
 *     - an axis < 2 gives 0 proposals (the notebook's edge slices are empty: NaN, then a TypeError);
 *     - while max_val is unset the 0.7 max_val clause is false (the notebook raises a TypeError when its first diff is exactly
 *       thresh);
 *     - the loop stops when an iteration would repeat the previous one's (loc, diff) exactly -- a peak on the last plane of an axis
 *       that the half-open box never clears: the notebook repeats it forever, so the proposals are the notebook's with the repeats
 *       removed;
 *     - at most max_proposals records and max_iters iterations.
 *   margin 1..64 (an edge slice holds <= 128 cells); the grid must be finite.  Workspace: cppf_scene_proposals_workspace_bytes()
 *   (two grid copies and a table of one (max, first index) per 8^3 cells: one workgroup runs the loop and rescans only the tiles
 *   a suppressed box touches).
 *
 * cppf_segment_instance (cell 11, "unsupervised instance segmentation"): from the back-vote survivors of one proposal
 *   (surv_mask device u8[n_pairs], cppf_backvote* at the proposal's centre): point_mask[n] = (n is an endpoint of more than
 *   min_contrib survivors, pairs (i, i) counting twice), then the survivors with either endpoint in the mask, in pair order:
 *   pairs_out device i32[n_pairs] (positions in the pair list), count device i32[1].  Integer atomics: the same result on every
 *   run.  point_idxs device i32[n_pairs,2]; workspace >= cppf_segment_instance_workspace_bytes().  An endpoint outside
 *   [0, n_points) is not counted and is in no instance; the pair's other endpoint counts as usual.
 * ------------------------------------------------------------------------------------------- */
int cppf_pair_filter_distinct(const float* pc, const float* nrm, const void* point_idxs, int idx_is_i64, int64_t n_points,
                              int64_t n_pairs, uint8_t* keep, void* stream);
size_t cppf_gaussian_filter3d_workspace_bytes(int gx, int gy, int gz);
int cppf_gaussian_filter3d(const float* grid, float* out, int gx, int gy, int gz, const double* weights, int radius,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_scene_proposals_workspace_bytes(int gx, int gy, int gz);
int cppf_scene_proposals(const float* grid, int gx, int gy, int gz, const double* weights, int radius, float thresh, int margin,
                         int max_proposals, int max_iters, int32_t* loc, float* value, float* diff, int32_t* count,
                         float* smoothed_out, void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_segment_instance_workspace_bytes(int64_t n_points, int64_t n_pairs);
int cppf_segment_instance(const int32_t* point_idxs, const uint8_t* surv_mask, int64_t n_pairs, int64_t n_points, int min_contrib,
                          uint8_t* point_mask, int32_t* pairs_out, int32_t* count, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * The per-proposal stage of a scene for ALL proposals in one pass over the pair list (csrc/scene_multi.hip; additive, ABI version
 * unchanged).  What K calls of cppf_backvote_ws + cppf_segment_instance compute, with the pair list, the pairs' points and the
 * pairs' frames read once instead of K times.
 *
 * cppf_backvote_multi: the back-vote of models/voting.py:74-112 at n_centers (1..32) centres.  Bit k of surv_bits[p] equals, bit
 *   for bit, the mask cppf_backvote_ws writes for pair p at centers[k] (always adaptive, bounds [0, dim-1), the first passing
 *   rotation in index order decides, degenerate pairs give 0); bits >= n_centers are 0.  centers device f32[n_centers,3];
 *   surv_bits device u32[n_ppfs], cleared by the call and filled with integer OR atomics: the same words on every run.
 *   vote_workspace: as for cppf_backvote_ws (may be NULL).  CPPF_EINVAL: n_centers outside 1..32, n_rots outside 1..CPPF_MAX_ROTS,
 *   a dim < 1, a null pointer, n_ppfs < 0 or n_ppfs >= 2^27 (a queue entry packs the pair with the 5 bits of k).  n_ppfs == 0
 *   returns 0 and launches nothing.
 *
 * cppf_segment_instances: cppf_segment_instance on every bit.  point_masks device u8[n_centers,n_points]: row k is the point_mask
 *   of bit k.  The kept pairs of proposal k (positions in the pair list, in pair order) are pairs_out[offsets[k] .. offsets[k+1]);
 *   offsets device i32[n_centers+1] always holds the true prefix sums.  pairs_out device i32[capacity]: when offsets[n_centers] >
 *   capacity nothing is written at or beyond `capacity` and the call returns 0 -- the caller reads offsets and repeats the call
 *   with a buffer of offsets[n_centers] entries.  The endpoint counts are integer atomics into a [n_centers,n_points] table in ONE
 *   pass over the pair list (pairs (i, i) count twice); the results are the same on every run.  Bits >= n_centers of surv_bits are
 *   ignored.  CPPF_EINVAL: n_centers outside 1..32, n_points outside 1..2^31-1, negative sizes, null pointers; CPPF_EUNSUPPORTED:
 *   n_pairs n_centers > 2^31-1 (the offsets are int32); workspace >= cppf_segment_instances_workspace_bytes().
 * ------------------------------------------------------------------------------------------- */
int cppf_backvote_multi(const float* points, const float* outputs, const int32_t* point_idxs, const float* corner, float res,
                        int64_t n_ppfs, int n_rots, int gx, int gy, int gz, const float* centers, int n_centers, float tol,
                        uint32_t* surv_bits, const void* vote_workspace, void* stream);
size_t cppf_segment_instances_workspace_bytes(int64_t n_points, int64_t n_pairs, int n_centers);
int cppf_segment_instances(const int32_t* point_idxs, const uint32_t* surv_bits, int64_t n_pairs, int64_t n_points, int n_centers,
                           int min_contrib, uint8_t* point_masks, int32_t* pairs_out, int64_t capacity, int32_t* offsets,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance clouds of the proposals (csrc/instances.hip; additive, ABI version unchanged): what connects the mask-free path's point
 * masks to the instance path.  A mask of cppf_segment_instances speaks of the SPARSE cloud (one point per voxel of 4 res); the
 * instance path wants the DENSE cloud's points (res).  `owner` maps the one onto the other: owner[i] = the position in the sparse
 * cloud of the point that represents dense point i's voxel, negative = none (cppf_amd.scene_stage.voxel_owner computes it once per
 * cloud with the fp64 true division of cppf_voxel_dedupe).
 *
 * cppf_gather_instances: ONE pass over the dense cloud for n_props (1..32) proposals.
 *   in:  hi, hi_nrm device f32[n_dense,3]; owner device i32[n_dense]; masks device u8[n_props,n_sparse] (non-zero = member: the
 *        point_masks of cppf_segment_instances).
 *   out: member device u32[n_dense]: bit k of member[i] is set iff 0 <= owner[i] and masks[k][owner[i]] != 0; bits >= n_props are 0.
 *        offsets device i32[n_props+1]: the exclusive prefix of the proposals' member counts -- always complete.
 *        pts, nrm device f32[capacity,3], src device i32[capacity]: rows offsets[k] .. offsets[k+1] hold hi[i], hi_nrm[i] and i for
 *        the members i of proposal k in increasing i (what hi[member_k] gives on the host; a point in several masks is copied
 *        into each).  Nothing is written at or beyond row `capacity`: when offsets[n_props] > capacity the call still returns 0 and
 *        the caller repeats it with buffers of offsets[n_props] rows.  n_dense rows hold any one proposal.
 *        chunk_counts device i32[CPPF_GATHER_COUNTS(n_props, n_dense)]: the members per proposal and chunk of CPPF_GATHER_CHUNK
 *        dense points, proposal-major -- the call's only intermediate, a typed argument and not a workspace: n_props *
 *        ceil(n_dense / CPPF_GATHER_CHUNK) integers, overwritten by every call.
 *   Two launches on `stream` (memberships and counts from wave ballots; the copy, every workgroup summing the counts in front of
 *   its own), no atomics, no read-back: the same words on every run.
 *   An owner[i] >= n_sparse is never followed.  It is found on the stream and reported as offsets[n_props] = -1 (offsets[k] = 0
 *   below it); pts, nrm and src are then left untouched and member is unspecified -- the way cppf_voxel_dedupe reports a cloud
 *   it refuses.  The return value is still 0: the caller reads offsets.
 *   CPPF_EINVAL: n_props outside 1..32, a negative size, n_dense or n_props n_dense or n_sparse > 2^31-1 (offsets, src and owner are
 *   int32), a null pointer (pts / nrm / src may be NULL with capacity 0; every input and member / chunk_counts with n_dense 0).
 *   CPPF_EUNSUPPORTED: more than CPPF_GATHER_MAX_CHUNKS chunks (8 388 608 dense points, cppf_frame_cloud_dyn's frame bound).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_GATHER_CHUNK 1024
#define CPPF_GATHER_MAX_CHUNKS 8192
#define CPPF_GATHER_COUNTS(n_props, n_dense) ((int64_t)(n_props) * (((int64_t)(n_dense) + CPPF_GATHER_CHUNK - 1) / CPPF_GATHER_CHUNK))
int cppf_gather_instances(const float* hi, const float* hi_nrm, const int32_t* owner, const uint8_t* masks, int n_props,
                          int64_t n_sparse, int64_t n_dense, int64_t capacity, uint32_t* member, int32_t* offsets, float* pts,
                          float* nrm, int32_t* src, int32_t* chunk_counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Segment clouds (csrc/instances.hip; additive, ABI version unchanged): the dense cloud packed by a per-point LABEL -- the segments
 * of cppf_depth_segments as instance clouds, without the scene stage in between.  cppf_gather_instances takes at most 32 possibly
 * overlapping proposals as mask rows through an owner map; segments are up to CPPF_SEGMENTS_MAX disjoint labels of the dense points
 * themselves, so one call serves a whole frame.
 *
 * cppf_gather_segments: a stable partition of the dense cloud by label.
 *   in:  hi, hi_nrm device f32[n_dense,3]; labels device i32[n_dense] (SceneCloud.hi_labels).  A label outside [0, n_segments) --
 *        -1 included -- belongs to no segment: the point is skipped, never an error.
 *   out: offsets device i32[n_segments+1]: the exclusive prefix of the segments' point counts -- always complete.
 *        pts, nrm device f32[capacity,3], src device i32[capacity]: rows offsets[s] .. offsets[s+1] hold hi[i], hi_nrm[i] and i for
 *        the points with labels[i] == s in increasing i (what hi[labels == s] gives on the host).  Nothing is written at or beyond
 *        row `capacity`: when offsets[n_segments] > capacity the call still returns 0.  Segments are disjoint: n_dense rows always
 *        suffice.  pts / nrm / src may be NULL with capacity 0 (a count-only call).
 *        bounds NULL or device f32[n_segments,6] = {min x, y, z, max x, y, z} over the segment's points whose three coordinates
 *        are all finite, in the order of the sign-magnitude integer key (-0.0 lies below +0.0); a segment with no such point gets
 *        {+inf, +inf, +inf, -inf, -inf, -inf}.
 *        chunk_counts device i32[CPPF_GATHER_COUNTS(n_segments, n_dense)]: the call's only intermediate, a typed argument and not a
 *        workspace -- CHUNK-major (n_segments integers per chunk of CPPF_GATHER_CHUNK points); after the call entry [c][s] holds
 *        segment s's points in the chunks before c.  Overwritten by every call.
 *   Four launches on `stream` (per-chunk counts from wave ballots; their prefix over the chunks, per label; the prefix of the
 *   totals; the copy), no host synchronisation, no read-back, no floating-point atomics -- the bounds are integer min / max on the
 *   floats' bits, which do not depend on order -- so every output word is the same on every run, and the call can be captured in a
 *   graph.  n_dense = 0: one launch that writes zero offsets and the empty bounds.
 *   CPPF_EINVAL: n_segments outside 1..CPPF_GATHER_SEGMENTS_MAX, a negative size, n_dense > 2^31-1, a null pointer (pts / nrm / src
 *   may be NULL with capacity 0; every input and chunk_counts with n_dense 0).
 *   CPPF_EUNSUPPORTED: more than CPPF_GATHER_MAX_CHUNKS chunks.
 * ------------------------------------------------------------------------------------------- */
#define CPPF_GATHER_SEGMENTS_MAX 1024            /* = CPPF_SEGMENTS_MAX */
int cppf_gather_segments(const float* hi, const float* hi_nrm, const int32_t* labels, int n_segments, int64_t n_dense,
                         int64_t capacity, int32_t* offsets, float* pts, float* nrm, int32_t* src, float* bounds,
                         int32_t* chunk_counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training views (utils/dataset.py:103-207, csrc/raster.hip): the pyrender `RenderFlags.DEPTH_ONLY` render of one mesh through
 * the dataset's PinholeCamera (:108-138), and the covered pixels as the dataset's point cloud.  Parity with pyrender is UNPINNED
 * (pyrender and its 24-bit depth buffer are not part of the project); the definition below is, to the operation, and
 * tests/mesh_ref.py restates it in numpy bit for bit.  All fp32 arithmetic is IEEE single with no contraction
 * (-ffp-contract=off), divisions correctly rounded.
 *
 * cppf_raster_depth
 *   verts device f64[n_verts,3] (model frame), faces device i32[n_faces,3], model_view_host HOST f64[12] = rows 0..2 of the
 *   row-major 4x4 model-view matrix M (NULL = identity).  Camera frame: OpenGL, the camera looks down -z.
 *   1. Transform (fp64, then rounded):  c_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3];  X = (float)c_0, Y = (float)c_1,
 *      d = -(float)c_2 (view depth).  A face index outside [0, n_verts) makes the call fail with CPPF_EINVAL.
 *   2. Near plane (znear; pyrender's default 0.05): vertex inside iff d >= zn (zn = (float)znear).  Sutherland-Hodgman over the
 *      edges (v0,v1), (v1,v2), (v2,v0): an inside vertex is kept; an edge with one end inside adds the point
 *      t = (a.d - zn) / (a.d - b.d), x = a.x + t (b.x - a.x), y likewise, d = zn, with a the INSIDE end.  The 3 or 4 vertices p0..
 *      are fanned: (p0,p1,p2) and (p0,p2,p3).  Nothing is projected through w <= 0; a triangle wholly in front of the plane
 *      yields nothing.
 *   3. Projection (P[0][0] = 2 fx / W, P[1][1] = 2 fy / H, no principal-point offset, infinite far plane), GL window coordinates
 *      (y UP): p00 = (float)(2.0 * fx / W), p11 = (float)(2.0 * fy / H), hw = 0.5f * W, hh = 0.5f * H;
 *      sx = ((p00 * x) / d + 1.0f) * hw;  sy = ((p11 * y) / d + 1.0f) * hh;  i = 1.0f / d.
 *   4. Orientation: A = (sx1 - sx0) * (sy2 - sy0) - (sx2 - sx0) * (sy1 - sy0).  A > 0 = CCW in window coordinates (y up) = front
 *      face (CW in the y-down image).  cull_back != 0: drop unless A > 0.  cull_back == 0: A < 0 swaps v1 and v2 (and their i)
 *      and negates A.  Then anything with !(A > 0) (zero area, NaN) covers nothing.
 *      ASSUMPTION: pyrender's Mesh.from_trimesh gives an untextured trimesh a single-sided material, so pyrender culls back
 *      faces with GL's default CCW front face.  pyrender's source is not part of the project; cull_back = 0 renders both sides.
 *   5. Bbox (decides which pixels are tested, so it is part of the definition): clampf(v, hi) = fminf(fmaxf(v, -1), hi);
 *      c0 = max(0, (int)floorf(clampf(min sx - 1, W))), c1 = min(W-1, (int)floorf(clampf(max sx + 1, W))); j0, j1 likewise from
 *      sy and H.  Pixel (col c, row r; row 0 at the top) is tested when c0 <= c <= c1 and j0 <= H-1-r <= j1.
 *   6. Coverage at the pixel centre px = c + 0.5f, py = (H - 1 - r) + 0.5f, with E(a,b) = (bx - ax) * (py - ay) - (by - ay) *
 *      (px - ax):  w0 = E(v1,v2), w1 = E(v2,v0), w2 = E(v0,v1).  Covered iff every w_k > 0, or w_k == 0 on a top-left edge:
 *      edge a->b is top-left iff (by - ay) < 0, or (by - ay) == 0 and (bx - ax) < 0 (left edges and horizontal top edges).
 *   7. Depth (1/d affine in screen space): d = ((w0 + w1) + w2) / ((w0 * i0 + w1 * i1) + w2 * i2).  The pixel keeps the MINIMUM
 *      over the fragments that cover it (independent of order); background is 0.0f, as pyrender returns it.  depth: device
 *      f32[H,W], every pixel written.
 *   Limits: 1 <= n_faces <= 2^28, W, H <= 8192.  The work is binned into 16x16 tiles; the bin list holds max_bin_entries
 *   (primitive, tile) pairs (<= 2^31 - 1).  Workspace: cppf_raster_workspace_bytes(n_faces, W, H, max_bin_entries); its first 8
 *   bytes hold the status {code, bin entries needed} of the last call.  When the bin list is too small (or a face index is out
 *   of range) every depth pixel is NaN and the status code is CPPF_ECAPACITY (CPPF_EINVAL): no fragment is dropped silently.
 *   sync != 0: the call waits for its stream and RETURNS that code; sync == 0: it returns at once and the caller reads the
 *   status words from the workspace.
 *
 * cppf_depth_points (:203-207 with utils/util.py:598-631): the pixels with depth > 0 in row-major order (np.where), through
 *   kinv_host (HOST f64[9], row-major inv(K); the dataset's K = [[591.0125,0,320],[0,590.16775,240],[0,0,1]]) with
 *   cppf_backproject's arithmetic, xyz = (fma(k01, v, k00 u) + k02, ...), (X, Y, Z) = xyz * z / xyz.z; backproject's x/y negation
 *   and the dataset's x/z negation give pts = (X, -Y, -Z) device f64[H*W,3].  u, v are the INTEGER pixel coordinates while the
 *   render samples pixel centres: the dataset's half-pixel shift, kept.  pix device i32[H*W] = r*W + c, count device i32[1].
 *   H*W <= 8192 * 1024; workspace >= cppf_depth_points_workspace_bytes(H, W).
 *
 * cppf_raster_instances: K posed instances of several meshes in ONE depth image, with the instance that won each pixel -- the
 *   multi-object frames of cppf_amd/mesh_frames.py.  One binned pass over all instances' triangles.
 *   verts device f64[V,3] and faces device i32[F,3] of all meshes, concatenated; face indices are LOCAL to their mesh.
 *   mesh_vert_off_host / mesh_face_off_host HOST i64[n_meshes+1] (first entry 0, every mesh with >= 1 vertex and >= 1 face),
 *   inst_mesh_host HOST i32[K] = the mesh each instance draws (a mesh may be drawn many times), model_views_host HOST f64[K,12] =
 *   rows 0..2 of each instance's model-view matrix, as cppf_raster_depth takes its one.  The call copies the four host tables
 *   into its workspace before it returns.  fx .. sync, workspace and stream: cppf_raster_depth's.
 *   Definition: steps 1-7 above apply unchanged to every (instance, face) with that instance's matrix.  A pixel keeps the MINIMUM
 *   depth over all fragments of all instances, and labels (device i32[H,W]) the index of the instance that produced it; on equal
 *   depth the LOWEST instance index wins, so neither image depends on the order of execution.  Background: depth 0.0f, label -1.
 *   Hence depth = the element-wise minimum over covered pixels of the K cppf_raster_depth renders, labels = the first arg-min,
 *   and K = 1 gives cppf_raster_depth's image bit for bit (both entry points run the same device functions).
 *   Failure: a face index outside its mesh's vertex range -> CPPF_EINVAL, a bin list that is too small -> CPPF_ECAPACITY, both
 *   through the status words as above; every depth pixel is then NaN and every label -1.  An inst_mesh entry outside
 *   [0, n_meshes), an offset table that does not start at 0 or does not increase, or K < 1 returns CPPF_EINVAL from the host
 *   before anything is launched.
 *   Limits: 1 <= K <= 65536; Q = the sum over the instances of faces(inst_mesh[k]) <= 2^28; W, H <= 8192; max_bin_entries
 *   <= 2^31 - 1.  Workspace: cppf_raster_instances_workspace_bytes(K, Q, n_meshes, W, H, max_bin_entries), status words first.
 * ------------------------------------------------------------------------------------------- */
size_t cppf_raster_workspace_bytes(int64_t n_faces, int W, int H, int64_t max_bin_entries);
int cppf_raster_depth(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const double* model_view_host,
                      double fx, double fy, int W, int H, double znear, int cull_back, float* depth, int64_t max_bin_entries, int sync,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_raster_instances_workspace_bytes(int n_instances, int64_t n_inst_faces, int n_meshes, int W, int H, int64_t max_bin_entries);
int cppf_raster_instances(const double* verts, const int32_t* faces, const int64_t* mesh_vert_off_host, const int64_t* mesh_face_off_host,
                          int n_meshes, const int32_t* inst_mesh_host, const double* model_views_host, int n_instances, double fx,
                          double fy, int W, int H, double znear, int cull_back, float* depth, int32_t* labels, int64_t max_bin_entries,
                          int sync, void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_depth_points_workspace_bytes(int H, int W);
int cppf_depth_points(const float* depth, int H, int W, const double* kinv_host, double* pts, int32_t* pix, int32_t* count,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh statistics (gen_stats.py, csrc/mesh_stats.hip): the per-mesh figures a new category's config is written from -- surface
 * samples of each mesh, then the bounding box and the maxima of generate_target's targets_tr (utils/dataset.py:20-36) over random
 * pairs.  Both calls take a batch of M meshes (one launch sequence per batch) and have no host synchronisation.  Parity with
 * Open3D's SamplePointsUniformly (its mt19937 stream, its summation) is UNPINNED: Open3D is not part of the project.  The
 * definition below is, to the operation, and tests/mesh_stats_ref.py restates it in numpy bit for bit.  All arithmetic is IEEE
 * double with no contraction (-ffp-contract=off); division and sqrt are correctly rounded.
 *
 * Two facts keep the device side small:
 *   - the normals only feed target_rot_aux, which gen_stats.py discards: the statistics need no normals;
 *   - up_sym / right_sym / z_right change target_rot only, never targets_tr: the statistics need no flags (they matter only once
 *     written into a config).
 *
 * Uniforms: Philox-4x32-10 (csrc/cppf_math.h) keyed by `seed` (key = {seed lo, seed hi}).  Counter {index, mesh, stream, 0} with
 * mesh = first_mesh + the mesh's position in the batch, stream 2 = surface points (index = point k), stream 3 = pairs (index =
 * pair p); streams 0 and 1 are cppf_sample_pairs'.  So a mesh's draws depend on (seed, first_mesh + m) alone: a batch of M equals
 * M calls of one mesh with first_mesh = 0 .. M-1.  u53(w0, w1) = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, in [0, 1).
 *
 * cppf_surface_sample_batch (Open3D's SamplePointsUniformly): n_points points per mesh.
 *   verts device f64[V,3] and faces device i32[F,3] of all meshes, concatenated; face indices are LOCAL to their mesh.
 *   vert_off_host / face_off_host HOST i64[M+1], starting at 0: mesh m has vertices [vo[m], vo[m+1]) and faces [fo[m], fo[m+1]),
 *   at least one of each and at most 2^31 - 1.
 *   1. Area (Open3D's formula): x = v0 - v1, y = v0 - v2, c = x cross y (c0 = x1 y2 - x2 y1, c1 = x2 y0 - x0 y2,
 *      c2 = x0 y1 - x1 y0), a_t = 0.5 * sqrt((c0 c0 + c1 c1) + c2 c2).  A face index outside its mesh gives NaN and status bit 2.
 *   2. Total S, blocked: K = ceil(F / 1024); block l (0..1023) holds faces [l K, min(F, (l+1) K)); s_l = ((0 + a) + a) ... left to
 *      right over its block, S = ((0 + s_0) + s_1) ... + s_1023.  S not in (0, inf) (every face degenerate, or a NaN / inf
 *      coordinate) sets status bit 1.
 *   3. q_t = a_t / S.  Cumulative area, blocked as in 2: T_l = ((0 + q) + q) ... over block l, B_0 = 0, B_l = B_l-1 + T_l-1, and
 *      within block l C_t = ((B_l + q_first) + ...) + q_t left to right.  For F <= 1024 (K = 1) this is Open3D's serial chain.
 *   4. Counts (Open3D's rule): E_t = min(N, round(C_t * N)) with round = halves away from zero (std::round, not numpy's
 *      round-half-even), E_{F-1} = N.  Point k lies on the FIRST face t with E_t > k (Open3D's loop, which moves on to the next
 *      face once its point index has reached round(C_t N)).  E may DECREASE by one behind a block boundary: B_l+1 = B_l + T_l has
 *      T_l summed from zero while the last C of block l was summed from B_l, the two roundings can differ by an ulp, and the lower
 *      value stays for as long as zero-area faces follow.  So "first" is meant literally and is not a bisection of E; with
 *      R_t = max(E_0 .. E_t) face t gets the points [R_{t-1}, R_t) (R_{-1} = 0), and the device stores R.  Zero-area faces get
 *      none.
 *   5. Point k on face (v0, v1, v2): {w} = Philox({k, mesh, 2, 0}), r1 = u53(w.x, w.y), r2 = u53(w.z, w.w), s = sqrt(r1),
 *      a = 1 - s, b = s * (1 - r2), c = s * r2, p_j = (a * v0_j + b * v1_j) + c * v2_j.
 *   points device f64[M, n_points, 3]; face_ids device i32[M, n_points] (local face index; NULL = not written); status device
 *   i32[M] (0 = sampled).  A mesh with a status bit gets NaN points and face id -1; the other meshes are unaffected.  Bit 2 never
 *   comes alone: the NaN area of the offending face makes S NaN, so such a mesh has status 3.  A NaN / inf vertex that no face
 *   references changes nothing.
 *   n_points <= 2^31 - 1, first_mesh + M <= 2^32.  Workspace >= cppf_surface_sample_workspace_bytes(M, fo[M]).  The offsets are
 *   copied to the device inside the call.
 *
 * cppf_mesh_vote_stats_batch (the loop body of gen_stats.py): points device f64[M, n_points, 3] (e.g. the samples above).
 *   1. Bounding box lo, hi per axis, centre c = (lo + hi) / 2; the centred maximum / minimum hc = hi - c, lc = lo - c (rounding is
 *      monotonic, so these are the max / min of the centred points); e = hc - lc, diag = sqrt((e0 e0 + e1 e1) + e2 e2).
 *   2. Pair p < n_pairs: {w} = Philox({p, mesh, 3, 0}), i = (w.x * N) >> 32, j = (w.y * N) >> 32 (cppf_sample_pairs' rule; i == j
 *      is kept, as np.random.randint keeps it).  a = P_i - c, b = P_j - c (per coordinate), d = a - b, u = d / (sqrt((dx dx +
 *      dy dy) + dz dz) + 1e-7), proj = (ax ux + ay uy) + az uz, o = a - proj u, dist2o = sqrt((ox ox + oy oy) + oz oz).
 *   3. Max of |proj| and of dist2o over the pairs (exact in any order), then cast to float32 (the reference's max over float32
 *      values: the cast is monotonic).
 *   stats device f64[M,6] = {diag, max|proj| (a float32 value), max dist2o (a float32 value), hc_x, hc_y, hc_z}; status device
 *   i32[M]: 1 = a non-finite point (that row is NaN).  n_pairs <= 2^32 - 1.  Workspace >= cppf_mesh_vote_stats_workspace_bytes.
 * ------------------------------------------------------------------------------------------- */
size_t cppf_surface_sample_workspace_bytes(int n_meshes, int64_t n_faces_total);
int cppf_surface_sample_batch(const double* verts, const int32_t* faces, const int64_t* vert_off_host, const int64_t* face_off_host,
                              int n_meshes, int64_t n_points, unsigned long long seed, int64_t first_mesh, double* points,
                              int32_t* face_ids, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
size_t cppf_mesh_vote_stats_workspace_bytes(int n_meshes, int64_t n_points, int64_t n_pairs);
int cppf_mesh_vote_stats_batch(const double* points, int n_meshes, int64_t n_points, int64_t n_pairs, unsigned long long seed,
                               int64_t first_mesh, double* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pose evaluation (nocs/eval.py -> utils/util.py:181-255,342-416,470-517, csrc/pose_eval.hip): the per-pair box IoU and pose
 * errors and the two greedy matchings of compute_degree_cm_mAP, for a whole result set in three launches with no host
 * synchronisation.  The arithmetic is cppf_amd/evaluation.py's (its host path is the checker), in IEEE double without contraction.
 *
 * cppf_pose_eval_pairs: M work pairs (pairs device i32[M,2] = {prediction index, ground-truth index}).
 *   pred_RT / gt_RT device f64[.,4,4] (row-major; the last row is not read), pred_scales / gt_scales device f64[.,3], gt_up_sym
 *   device i32[n_gt], sweep device i32[M] (non-zero: the up-symmetry sweep applies to this pair's IoU -- the host sets it where the
 *   classes agree and the ground truth is up-symmetric).  Outputs iou device f64[M], err device f64[M,2] = {degrees, centimetres}.
 *   - A work item is (pair, rotation k): 20 for a swept pair (box 1 = RT_1 @ rot_y(2 pi k / 20), the cos / sin table the host's libm
 *     gives), 1 otherwise; a swept pair's IoU is the maximum over k (taken with an integer max on the bits: exact in any order).
 *   - Box of (RT, s): R = RT[:3,:3] / cbrt(det), axes = the normalised columns, half extents = 0.5 s * column norms, centre =
 *     RT[:3,3] (_frame).  Intersection volume: 1/3 of the sum over the faces of box 1 clipped by box 2's six half-spaces and vice
 *     versa of (n . x) * area (_faces, _clip, _flux, box_intersection_volume): a vertex is inside when n.x - d <= tol, tol = +1e-9 *
 *     (largest half extent of both boxes) while box 1's faces are clipped and -tol for box 2's; a crossing's t is clamped to [0,1];
 *     clipping of a face stops once fewer than 3 vertices are left.  IoU = v / (va + vb - v), and 0.0 when v <= 1e-9 min(va, vb)
 *     (_iou_frames).  A clipped quad has at most 10 vertices.
 *   - Errors (compute_RT_degree_cm_symmetry): with gt_up_sym the angle between the two y axes, else acos((trace(R1 R2^T) - 1) / 2),
 *     the cosine clamped to [-1,1], in degrees; 100 * |t1 - t2|.
 *   - A pair index outside [0, n_pred) x [0, n_gt) reads nothing and gives NaN in all three outputs.
 *   M <= CPPF_POSE_EVAL_MAX_PAIRS; M = 0 is a no-op.  Workspace >= cppf_pose_eval_pairs_workspace_bytes(M) (the work-item offsets).
 *
 * Groups: one (image, class) with its predictions [pred_off[g], pred_off[g+1]) -- in the order they claim, i.e. descending score as
 * the host sorts them -- and ground truths [gt_off[g], gt_off[g+1]) (device i32[G+1] each); its np x ng values (IoU, errors) are
 * rows [pair_off[g], pair_off[g] + np ng) of the pair arrays, prediction-major (device i64[G]).  At most
 * CPPF_POSE_EVAL_GROUP_CAP predictions and as many ground truths per group (the claimed set is one 32-bit mask; the reference's own
 * per-image tables stop at 20): a larger group, or one whose rows leave [0, n_pairs), gets -1 everywhere -- callers refuse it first.
 * Match tables are i32 with -1 = no match and hold indices LOCAL to the group; every entry of every group is written.
 *
 * cppf_pose_eval_match_iou (compute_3d_matches), one lane per (group, threshold): pred_match device i32[T, n_pred], gt_match
 *   device i32[T, n_gt].  IoUs are rounded to float32 before any comparison (the host's overlaps are float32).  Each prediction in
 *   turn takes the unclaimed ground truth with the largest IoU if that IoU is strictly above the threshold (the host's walk in
 *   descending IoU skips claimed ones and stops below the threshold, so only this one can match).
 *   TIE RULE: of several unclaimed ground truths with EQUAL float32 IoU the one with the HIGHER index is taken.  (The host's order
 *   among equals is whatever np.argsort does on its platform; it is not reproduced.)
 *
 * cppf_pose_eval_match_pose (compute_match_from_degree_cm), one lane per (group, degree threshold, shift threshold): pred_match
 *   device i32[D, S, n_pred], gt_match device i32[D, S, n_gt].  Each kept prediction in turn takes the unclaimed kept ground truth
 *   with the smallest degrees + centimetres among those with degrees <= threshold and centimetres <= threshold.
 *   TIE RULE: of several with EQUAL sum the one with the LOWER index is taken.
 *   keep_pred device i32[n_pred] / keep_gt device i32[n_gt]: an instance takes part when its entry is >= 0 -- one row of
 *   cppf_pose_eval_match_iou's tables, used where it lies (use_matches_for_pose); NULL: every prediction / ground truth takes part.
 * ------------------------------------------------------------------------------------------- */
#define CPPF_POSE_EVAL_GROUP_CAP 32
#define CPPF_POSE_EVAL_MAX_PAIRS 100000000
size_t cppf_pose_eval_pairs_workspace_bytes(int64_t n_pairs);
int cppf_pose_eval_pairs(const double* pred_RT, const double* pred_scales, int64_t n_pred, const double* gt_RT,
                         const double* gt_scales, const int32_t* gt_up_sym, int64_t n_gt, const int32_t* pairs, const int32_t* sweep,
                         int64_t n_pairs, double* iou, double* err, void* workspace, size_t workspace_bytes, void* stream);
int cppf_pose_eval_match_iou(const double* iou, const int32_t* pred_off, const int32_t* gt_off, const int64_t* pair_off, int n_groups,
                             const double* thresholds, int n_thresholds, int64_t n_pred, int64_t n_gt, int64_t n_pairs,
                             int32_t* pred_match, int32_t* gt_match, void* stream);
int cppf_pose_eval_match_pose(const double* err, const int32_t* pred_off, const int32_t* gt_off, const int64_t* pair_off, int n_groups,
                              const double* degree_thresholds, int n_degree, const double* shift_thresholds, int n_shift,
                              const int32_t* keep_pred, const int32_t* keep_gt, int64_t n_pred, int64_t n_gt, int64_t n_pairs,
                              int32_t* pred_match, int32_t* gt_match, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box NMS (sunrgbd/eval.py:13-35, csrc/box_nms.hip): greedy 3D non-maximum suppression over oriented boxes, every (image, class)
 * group of a result set in one call -- a memset and two launches, no host synchronisation.  Host side and checker:
 * cppf_amd/evaluation.py nms_3d.
 *
 * cppf_box_nms_batch: RT device f64[n,4,4] and scales device f64[n,3] in the form cppf_pose_eval_pairs reads (the rotation block
 *   may carry an isotropic scale, it is normalised by cbrt(det); the last row is not read), scores device f64[n].  group_off_host
 *   HOST i32[G+1], group_off[0] = 0, non-decreasing, group_off[G] = n: group g is the boxes [group_off[g], group_off[g+1]) -- one
 *   (image, class) set.  Empty groups are legal anywhere.
 *   Outputs: pick device i32[n]: the kept boxes of group g at pick[group_off[g] ..] in pick order, as indices WITHIN the group; the
 *   rest of the group's slots hold -1.  n_pick device i32[G].  iou_out NULL or device f64[sum_g m_g (m_g - 1) / 2]: every group's
 *   IoU upper triangle row by row (i < j), the groups in order -- there so that the IoUs can be pinned.
 *   THE RULE (sunrgbd/eval.py:21-35): the boxes of a group are visited by descending score; a visited box that is not suppressed is
 *   picked, and suppresses every later box whose IoU with it is STRICTLY greater than thresh (compared in fp64).
 *   TIE RULE: of boxes with EQUAL scores the one with the HIGHER index goes first -- what a stable ascending argsort read from the
 *   end gives.  (The reference's np.argsort leaves ties unspecified; they are this project's rule, pinned on nms_3d's host path.)
 *   An IoU that is NaN compares false and suppresses nothing (the reference's iou_3d returns 0 on an exception).
 *   The IoU of boxes i < j is the one cppf_pose_eval_pairs returns for the pair (i, j) with the same arrays on both sides and no
 *   sweep, bit for bit (csrc/pose_eval_box.h is shared).  Degenerate boxes (non-finite entries, a singular rotation block,
 *   non-positive extents, NaN scores) are the caller's duty, as there; nms_3d drops them before the upload.
 *   Returns CPPF_EINVAL for null pointers (iou_out aside), negative sizes, a table that decreases, does not start at 0 or does not
 *   end at n_boxes; CPPF_EUNSUPPORTED for a group of more than CPPF_BOX_NMS_GROUP_CAP boxes or more than 2^31 - 1 pairs in one call;
 *   CPPF_EWORKSPACE for a workspace below cppf_box_nms_workspace_bytes(n_boxes, n_groups) (the group, pair and word offset tables,
 *   uploaded inside the call, and the bit matrices: m rows of ceil(m / 64) 64-bit words per group, cleared by the call).
 *   n_boxes == 0 or n_groups == 0 returns 0 and launches nothing (no output is written).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_BOX_NMS_GROUP_CAP 1024
size_t cppf_box_nms_workspace_bytes(int64_t n_boxes, int n_groups);
int cppf_box_nms_batch(const double* RT, const double* scales, const double* scores, int64_t n_boxes, const int32_t* group_off_host,
                       int n_groups, double thresh, int32_t* pick, int32_t* n_pick, double* iou_out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Proposal verification (csrc/verify.hip; additive, ABI version unchanged): per-proposal evidence for up to 32 proposals of a
 * mask-free scene, from what cppf_backvote_multi and cppf_segment_instances have written.  The reference filters nothing, so the
 * definitions are this project's; tests/verify_ref.py restates them in numpy.  Host side: scene_stage.verify_proposals.
 * Both calls clear `counts`, count with integer atomics (the same words on every run), read nothing back, allocate nothing and can
 * be captured in a graph.
 *
 * cppf_proposal_support: one pass over the pair list.  point_idxs device i32[n_pairs,2]; surv_bits device u32[n_pairs] as
 *   cppf_backvote_multi writes them; point_masks device u8[n_props,n_points] as cppf_segment_instances writes them (non-zero =
 *   member).  counts device i32[n_props,4], for proposal k:
 *     within       pairs whose two endpoints are both members of mask k
 *     agree        those of `within` with bit k of surv_bits set
 *     cross        pairs with exactly one endpoint in mask k
 *     cross_agree  those of `cross` with bit k set
 *   An endpoint outside [0, n_points) is a non-member (the pair still counts through its other endpoint); a pair (i, i) with i in
 *   the mask is `within`, once; bits >= n_props of surv_bits are ignored.  n_pairs == 0 writes zeros and launches nothing more.
 *   The workspace holds one membership word per point (cppf_proposal_support_workspace_bytes).
 *   CPPF_EINVAL: n_props outside 1..32, n_points outside 1..2^31-1, n_pairs < 0 or >= 2^27, a null pointer (point_idxs and
 *   surv_bits may be null when n_pairs == 0), a workspace below cppf_proposal_support_workspace_bytes(n_points).
 *
 * cppf_box_support: one pass over the cloud.  points device f32[n_points,3]; centers f32[n_props,3]; axes f32[n_props,9]: the
 *   row-major 3x3 whose COLUMNS are the box axes (R of a pose); half f32[n_props,3]: half extents, padding included.  counts device
 *   i32[n_props,3], for proposal k:
 *     mask_pts     members of mask k
 *     mask_in_box  members that lie inside box k
 *     box_pts      all points inside box k
 *   Inside, in fp32, for a = 0, 1, 2: |d.x A[0][a] + d.y A[1][a] + d.z A[2][a]| <= half[a] with d = p - c, the products summed left
 *   to right without contraction.  A point with a non-finite coordinate is inside no box; a box with a NaN entry or a negative half
 *   extent holds no point.  CPPF_EINVAL: n_props outside 1..32, n_points outside 1..2^31-1, a null pointer.
 * ------------------------------------------------------------------------------------------- */
size_t cppf_proposal_support_workspace_bytes(int64_t n_points);
int cppf_proposal_support(const int32_t* point_idxs, const uint32_t* surv_bits, const uint8_t* point_masks, int64_t n_pairs,
                          int64_t n_points, int n_props, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int cppf_box_support(const float* points, const uint8_t* point_masks, const float* centers, const float* axes, const float* half,
                     int64_t n_points, int n_props, int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene training (csrc/scene_train.hip; additive, ABI version unchanged): what a training step on a whole labelled frame needs
 * besides the encoders -- a pair draw that yields same-instance pairs, and the targets of utils/dataset.py:27-60,229-246 for many
 * instances in one pass.  The reference trains on one object at a time, so the definitions are this project's;
 * tests/scene_training_ref.py restates them in numpy.  Host side: cppf_amd/scene_training.py.  Neither call takes a workspace,
 * allocates, synchronises with the host or uses atomics: both can be captured in a graph.
 *
 * The labelled cloud: inst device i32[n_points], the instance each point belongs to, -1 (or any value outside [0, n_inst)) =
 * background.
 *
 * The stratified draw.  members device i32[M]: the points of the TARGET category's instances, grouped by instance, ascending within
 *   a group; seg_off device i32[n_inst + 1] into members (an instance of another category has an empty segment); M = seg_off[n_inst]
 *   is read on the device; members_capacity = the entries the members buffer holds (>= M; 0 with a null pointer when there is none).
 *   idx device i32[n_pairs,2], 8-byte aligned.
 *   Pair p: {w} = Philox-4x32-10({p, 0, 4, 0}, key = seed) -- stream 4; streams 0..3 are taken (the uniform pair draw, the mesh
 *   statistics).  For p < n_pos_pairs and M > 0:  a = members[(w.x M) >> 32], k = inst[a], b = members[seg_off[k] + ((w.y L) >> 32)]
 *   with L = seg_off[k+1] - seg_off[k].  Otherwise a = (w.x N) >> 32, b = (w.y N) >> 32, the uniform draw's rule.  a == b is kept.
 *   A pair's draw depends on (seed, p) alone.  Lists that break the promises above (M above members_capacity, a member outside the cloud, a
 *   label without a segment, offsets outside [0, M]) give that pair the uniform rule and never an out-of-bounds read.
 *   CPPF_EINVAL: n_pairs outside 0..2^31-1, n_pos_pairs outside 0..n_pairs, and with n_pairs > 0: n_inst < 1, n_points outside
 *   1..2^31-1, a null pointer (members aside while its capacity is 0), a misaligned idx.
 *
 * The targets.  points / normals device f32[n_points,3]; idx device i32[n_pairs,2]; table device f32[n_inst,12] = {centre, up axis,
 *   right axis, scale target} per instance (the scale target, log(half extents) - log(scale_mean), is not read by the kernel: the
 *   loss gathers it by pair_inst); flags device i32[n_inst]: bit 0 = the instance is of the target category, bit 1 = up_sym, bit 2 =
 *   right_sym.  n_inst <= CPPF_SCENE_TRAIN_MAX_INSTANCES.  vote_range0 / vote_range1: the category's vote_range.
 *   Outputs, a structure of arrays over the pairs: kind u8[P], pair_inst i32[P], low u8[P,4] (4-byte aligned), w_low f32[P,4]
 *   (16-byte aligned), aux u8[P,2] (2-byte aligned); the head order is mu, nu, up, right.
 *   - POSITIVE (kind 1, pair_inst k): both points carry the same label k in [0, n_inst) and bit 0 of flags[k] is set.  In fp32, no
 *     contraction, dot products summed left to right: a = P_i - c, b = P_j - c, d = a - b, u = d / (|d| + 1e-7f), proj = a.u,
 *     dist2o = |a - proj u|, th_up = acosf(clamp(u.up, -1, 1)), under up_sym min(th_up, acosf(clamp(-(u.up), -1, 1))), th_right
 *     likewise with right_sym; n = N_i, negated when n.u < 0; aux = {n.up > 0, n.right > 0}.
 *     Values {clamp(proj + v0, 0, 2 v0), clamp(dist2o, 0, v1), th_up, th_right} over the maxima {2 v0, v1, pi, pi}; with interval =
 *     (float)(max / (bins - 1)) (fp64, rounded once):  x = value / interval, low = min(floor(x), bins - 2), w_low = 1 - (x - low):
 *     weight w_low on bin low and 1 - w_low on bin low + 1.
 *   - NEGATIVE (kind 0, pair_inst -1): every other pair, and a positive pair one of whose values is not finite.  low = {0, tr_bins -
 *     2, 0, 0}, w_low = {1, 0, 1, 1}, aux = {0, 0}: all nu weight on the farthest bin.
 *   - An index outside [0, n_points): kind 255, nothing is read for that pair, the other outputs as a negative pair's.
 *   CPPF_EINVAL: n_inst outside 1..32, bins outside 2..256, a vote range that is not positive, n_pairs outside 0..2^31-1, and with
 *   n_pairs > 0: n_points outside 1..2^31-1, a null pointer, a misaligned idx / low / w_low / aux.
 * ------------------------------------------------------------------------------------------- */
#define CPPF_SCENE_TRAIN_MAX_INSTANCES 32
int cppf_sample_scene_pairs(const int32_t* members, int64_t members_capacity, const int32_t* seg_off, int n_inst, const int32_t* inst,
                            int64_t n_points, int64_t n_pairs, int64_t n_pos_pairs, unsigned long long seed, int32_t* idx, void* stream);
int cppf_scene_pair_targets(const float* points, const float* normals, const int32_t* inst, int64_t n_points, const int32_t* idx,
                            int64_t n_pairs, const float* table, const int32_t* flags, int n_inst, double vote_range0,
                            double vote_range1, int tr_bins, int rot_bins, uint8_t* kind, int32_t* pair_inst, uint8_t* low,
                            float* w_low, uint8_t* aux, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth segments (csrc/segments.hip; additive, ABI version unchanged): what a depth frame says about its objects without any network
 * -- connected components of the depth image under a depth-discontinuity rule, and a RANSAC plane fit to cut the support surface
 * away first.  The reference has neither, so the definitions are this project's; tests/segments_ref.py restates them in numpy /
 * scipy.  Host side: cppf_amd/segments.py.  Neither call takes a workspace: all scratch is a defined output.  Neither allocates or
 * synchronises with the host; both use integer atomics only, so the same inputs give the same bits, and both can be captured in a
 * graph.
 *
 * cppf_depth_segments.  depth device [H,W]: the int16 bits of the uint16 millimetres, compared as UNSIGNED; valid device u8[H,W] or
 *   NULL.  Outputs, device: labels i32[H,W], comp_size i32[H,W], first i32[capacity], sizes i32[capacity], counts i32[4].
 *   All in 32-bit integers:
 *   - a pixel is LIVE when depth > 0 and (valid is NULL or valid[p] != 0);
 *   - two 4-neighbours a, b are LINKED when both are live and |za - zb| <= tol_mm + (slope_permille * min(za, zb)) / 1000 (floor);
 *   - a component is a connected component of that graph, its ROOT its smallest flat pixel index;
 *   - comp_size[p] = the size of p's component for a live pixel, 0 for a dead one;
 *   - a component is KEPT when size >= min_pixels and (max_pixels == 0 or size <= max_pixels); the S kept components are numbered
 *     0..S-1 by ascending root; labels[p] = that number for the pixels of kept components, -1 everywhere else;
 *   - first[s] = the root and sizes[s] = the size of kept component s; first[s] = -1 and sizes[s] = 0 for S <= s < capacity;
 *   - counts = {S, components of any size, live pixels, 0}.
 *   Overflow, S > capacity: counts and comp_size are as defined; the caller retries with a larger capacity.  (labels, first and
 *   sizes are then not to be relied on; this implementation writes -1 / -1 / 0 everywhere.)
 *   Every output is a function of the inputs alone: a root is a minimum and a number is a rank.
 *   CPPF_EINVAL: H or W < 1, H * W > 2^24, tol_mm outside 0..65535, slope_permille outside 0..1000, min_pixels < 1, max_pixels < 0,
 *   capacity outside 1..CPPF_SEGMENTS_MAX, a null pointer (valid aside).
 *
 * cppf_plane_ransac.  points device f32[n_points,3]; outputs, device: planes f32[n_hyp,4] (16-byte aligned), counts i32[n_hyp],
 *   best i32[2].  Hypothesis h: {w} = Philox-4x32-10({h, 0, 5, 0}, key = seed) -- stream 5; streams 0..4 are taken.  i_k = (w.k
 *   n_points) >> 32 for k = x, y, z name the points a, b, c.  In fp32, no contraction: e1 = b - a, e2 = c - a, n = e1 x e2 (each
 *   component two products and one subtraction), l = sqrtf((n.x n.x + n.y n.y) + n.z n.z).  DEGENERATE when !(l > 1e-12f), when any
 *   of the nine coordinates is not finite, or when the plane below is not finite (a cross product that overflowed).  Otherwise n = n /
 *   l, d = -((n.x a.x + n.y a.y) + n.z a.z), and all four are negated when d < 0: the origin is on the non-negative side.  A
 *   degenerate hypothesis has the plane {0, 0, 0, 0} and the count 0.
 *   counts[h] = the points with fabsf(((n.x p.x + n.y p.y) + n.z p.z) + d) <= thresh; a point with a non-finite coordinate is no
 *   inlier of any plane.  best = {the lowest h with the largest count among the hypotheses that are not degenerate, that count}, or
 *   {-1, 0} when every hypothesis is degenerate.
 *   CPPF_EINVAL: n_points outside 1..2^31-1, n_hyp outside 1..CPPF_PLANE_MAX_HYPOTHESES, a thresh that is not finite and >= 0, a
 *   null pointer, a misaligned planes.
 * ------------------------------------------------------------------------------------------- */
#define CPPF_SEGMENTS_MAX 1024
#define CPPF_PLANE_MAX_HYPOTHESES 1024
int cppf_depth_segments(const int16_t* depth, const uint8_t* valid, int H, int W, int tol_mm, int slope_permille, int min_pixels,
                        int max_pixels, int capacity, int32_t* labels, int32_t* comp_size, int32_t* first, int32_t* sizes,
                        int32_t* counts, void* stream);
int cppf_plane_ransac(const float* points, int64_t n_points, int n_hyp, float thresh, unsigned long long seed, float* planes,
                      int32_t* counts, int32_t* best, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Concave edges (csrc/concave.hip; additive, ABI version unchanged): the pixels of a depth frame across which the surface turns
 * TOWARDS itself -- where an object stands on its support or leans on a neighbour; an object's own edges are convex.  `edge == 0`,
 * ANDed into cppf_depth_segments' `valid`, cuts the components there (cppf_amd/segments.py: frame_segments(concave=)).  The
 * reference has nothing of the kind, so the definition is this project's; tests/concave_ref.py restates it in numpy and is held to a
 * loop-per-pixel brute force.  No workspace (`normal` carries the fits between the launches), no allocation, no host
 * synchronisation, integer atomics only: the same inputs give the same bits, and the call can be captured in a graph.
 *
 * cppf_concave_edges.  depth device [H,W]: the int16 bits of the uint16 millimetres, compared as UNSIGNED; valid device u8[H,W] or
 *   NULL; fx, fy, cx, cy: the pinhole intrinsics of the INTEGER pixel coordinates (u = column, v = row).  Outputs, device, every
 *   byte written: edge u8[H,W] (0 / 1), normal f64[H,W,3] (unit, or 0 0 0 where there is no fit), counts i32[4] = {edge pixels,
 *   pixels with a fit, live pixels, 0}.
 *   1. A pixel is LIVE when depth > 0 and (valid is NULL or valid[p] != 0).  z0 = the depth of a live pixel p.
 *   2. Window, in integers: lim = tol_mm + (slope_permille * z0) / 1000 (floor).  The pixel q at offset (du, dv), both in [-radius,
 *      radius], is ADMITTED when it lies inside the frame, is live and |zq - z0| <= lim * max(|du|, |dv|, 1); p admits itself.
 *      Over the admitted pixels, with dz = zq - z0: n, Su = sum du, Sv = sum dv, Suu = sum du du, Suv = sum du dv, Svv = sum dv dv,
 *      Sz = sum dz, Szu = sum dz du, Szv = sum dz dv.
 *   3. Least squares dz ~ c0 + a du + b dv by Cramer's rule on [[n,Su,Sv],[Su,Suu,Suv],[Sv,Suv,Svv]] (c0,a,b) = (Sz,Szu,Szv): the
 *      determinant D and the three numerator determinants are integers.  |dz| <= 65535 whatever tol_mm and slope_permille are (two
 *      uint16 depths), so at radius 8 |D| < 5.8e10 and every numerator is under 3.9e15 < 2^53 (tests/concave_ref.py:
 *      numerator_bound): int64 holds them and their conversion to fp64 is exact.  p HAS A PLANE when n >= min_count and D > 0; then
 *      c0, a, b are ONE fp64 division each, and c = ((double)z0 + c0) / 1000.0, am = a / 1000.0, bm = b / 1000.0 (metres, metres
 *      per pixel).  Without a plane c = am = bm = 0.
 *   4. In fp64, one rounding per operation, no contraction, in exactly this order: xu = (double)u - cx, yv = (double)v - cy;
 *      Pu = (c / fx + (xu * am) / fx, (yv * am) / fy, am);  Pv = ((xu * bm) / fx, c / fy + (yv * bm) / fy, bm)   (the tangents);
 *      N = Pu x Pv, each component two products and one subtraction: (Pu.y Pv.z - Pu.z Pv.y, Pu.z Pv.x - Pu.x Pv.z, Pu.x Pv.y -
 *      Pu.y Pv.x);  P = ((xu * c) / fx, (yv * c) / fy, c)   (the fitted surface point);
 *      N is negated when (N.x P.x + N.y P.y) + N.z P.z > 0 (so that it faces the camera);  l = sqrt((N.x N.x + N.y N.y) + N.z N.z).
 *   5. p HAS A FIT when l is finite and > 0 (c = am = bm = 0 gives l = 0); normal[p] = N / l (three divisions) then, 0 0 0 otherwise.
 *   6. A live pixel p is an EDGE when, for the horizontal (e = (1, 0)) or the vertical (e = (0, 1)) axis, m = p - step e and q = p +
 *      step e both lie inside the frame and have a fit, and with d = P(q) - P(m), g = N(q) - N(m):
 *      (d.x d.x + d.y d.y) + d.z d.z <= span_max * span_max,  (N(m).x N(q).x + N(m).y N(q).y) + N(m).z N(q).z < cos_max,  and
 *      (d.x g.x + d.y g.y) + d.z g.z < 0 -- the normals converge: the crease is concave.  Dead pixels are never edges; p itself
 *      needs no fit.
 *   CPPF_EINVAL (nothing is written): H or W < 1, H * W > 2^24, radius outside 1..CPPF_CONCAVE_MAX_RADIUS, step outside
 *   1..CPPF_CONCAVE_MAX_STEP, tol_mm outside 0..65535, slope_permille outside 0..1000, min_count < 3, cos_max outside (-1, 1),
 *   span_max not finite and > 0, fx or fy not finite and > 0, cx or cy not finite, a null pointer (valid aside).
 * ------------------------------------------------------------------------------------------- */
#define CPPF_CONCAVE_MAX_RADIUS 8
#define CPPF_CONCAVE_MAX_STEP 16
int cppf_concave_edges(const int16_t* depth, const uint8_t* valid, int H, int W, double fx, double fy, double cx, double cy, int radius,
                       int step, int tol_mm, int slope_permille, int min_count, double cos_max, double span_max, uint8_t* edge,
                       double* normal, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CPPF_H */
