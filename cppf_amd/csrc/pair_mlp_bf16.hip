// bf16 pair encoder for gfx950: the kernel of pair_mlp.hip with the hidden layers on the bf16 matrix instructions.  Opt-in
// (PPFEncoder.set_precision("bf16")); the fp32 kernel stays the default and is not touched by this file.
//
// Numerics (DESIGN.md "bf16 pair encoder"; tests/pair_bf16_ref.py is the CPU statement).  bf() = round to nearest even to bf16.
//   layer 0   fp32, exactly the fp32 kernel's: per-point tables TA / TB from pair_mlp.hip's point_proj kernels (fp32 layer-0 weights),
//             the 4 PPF inputs through one v_mfma_f32_16x16x4_f32 k-step -> fp32 pre-activations of fc1 and fc0
//   then      a0 = bf(relu(fc1_0));          x1 = fc2_0(a0) + b + fc0_0
//   layer 1   h = bf(x1); a = bf(relu(fc1(h) + b));  x2 = fc2(a) + b + x1            (residual: the unrounded fp32 x1)
//   layer 2   h = bf(x2); a = bf(relu(fc1(h) + b));  x3 = fc2(a) + b + (fc0(h) + b0)
//   final     logits = final(bf(x3)) + b
// All products are bf16 x bf16 (weights rounded once, by the packer), all accumulation, biases and residual adds fp32; the logits are
// fp32 and the decode (softmax weights, inverse-CDF draw, bin -> value, aux logits, log-scales) is the fp32 kernel's own code.
//
// Structure: as pair_mlp.hip -- lane l = (j = l & 15, g = l >> 4) of a wave serves pair j of a 16-pair block, everything transposed,
// D[out][pair].  After a 32-wide layer lane g holds outputs 16*ob + 4g + r (ob = 0, 1; r = 0..3) of its pair: converted pairwise to
// bf16 those eight values ARE the B operand of v_mfma_f32_16x16x32_bf16 for k-slots 8g .. 8g + 7, so the weights are packed with the
// k-slot (g, jj) holding feature 16*(jj >> 2) + 4g + (jj & 3) (pair_layout_bf16.h: k32) and layers chain with no lane movement and no
// LDS, as in the fp32 kernel.  After a 16-wide layer the four values 4g + r are the lane's four k-slots of v_mfma_f32_16x16x16_bf16 in
// natural order.  Per 16-pair tile: 4 fp32 MFMAs (layer 0) + 8 of the K = 32 form + 10 of the K = 16 form, against 88 fp32 ones.
#include "pair_mlp_common.h"
#include "pair_layout_bf16.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

extern "C" size_t cppf_pair_mlp_bf16_packed_bytes(int F, const int* dims, int n_res, int out_dim)
{
    if (!dims) return 0;
    return is_std(F, dims, n_res, out_dim) ? (size_t)BF16_PACKED * 4 : 0;
}

extern "C" int cppf_pair_mlp_bf16_pack(const float* params, const int64_t* offs, int F, const int* dims, int n_res, int out_dim,
                                       void* out)
{
    if (!params || !offs || !dims || !out) return CPPF_EINVAL;
    if (!is_std(F, dims, n_res, out_dim)) return CPPF_EUNSUPPORTED;
    if (offs[4] < 0 || offs[10] >= 0 || offs[16] < 0) return CPPF_EINVAL;  // fc0 on layers 0 and 2 only
    uint32_t* o = static_cast<uint32_t*>(out);
    for (int i = 0; i < BF16_PACKED; ++i) o[i] = bf16_pack_word(i, params, offs, out_dim);
    return 0;
}

struct PackOffsB { int64_t o[20]; };
__global__ __launch_bounds__(256) void pair_pack_bf16_kernel(const float* __restrict__ params, PackOffsB offs, int out_dim,
                                                             uint32_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < BF16_PACKED) out[i] = bf16_pack_word(i, params, offs.o, out_dim);
}
extern "C" int cppf_pair_mlp_bf16_pack_device(const float* params, const int64_t* offs, int F, const int* dims, int n_res,
                                              int out_dim, void* out, void* stream)
{
    if (!params || !offs || !dims || !out) return CPPF_EINVAL;
    if (!is_std(F, dims, n_res, out_dim)) return CPPF_EUNSUPPORTED;
    if (offs[4] < 0 || offs[10] >= 0 || offs[16] < 0) return CPPF_EINVAL;
    PackOffsB po;
    for (int i = 0; i < 20; ++i) po.o[i] = offs[i];
    hipLaunchKernelGGL(pair_pack_bf16_kernel, dim3((BF16_PACKED + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, po,
                       out_dim, static_cast<uint32_t*>(out));
    CPPF_CHECK_LAUNCH();
    return 0;
}

// ----------------------------------------------------------------------------- kernel
__device__ __forceinline__ f32x4 mfma32b(bf16x8 a, bf16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16b(bf16x4 a, bf16x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}
// bf() of the lane's 8 / 4 accumulator values: v_cvt_pk_bf16_f32, two values per instruction (left to the compiler: no builtin, and an
// asm statement is not counted as a VALU reader of an MFMA result -- see relu1 in pair_mlp_common.h)
__device__ __forceinline__ bf16x8 bf8(f32x4 lo, f32x4 hi)
{
    f32x8 v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_convertvector(v, bf16x8);
}
__device__ __forceinline__ bf16x4 bf4(f32x4 v) { return __builtin_convertvector(v, bf16x4); }
__device__ __forceinline__ bf16x8 ldw8(const float* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x4 ldw4(const float* p) { return *reinterpret_cast<const bf16x4*>(p); }

// ---- epilogues of one 16-pair block: L[ob] = the lane's 4 outputs 16*ob + 4*g .. of its pair (natural column order for the logits,
//      dec_col order for the decode).  The text of pair_mlp.hip's epilogue, which stays inline there: as a function shared by both
//      files it changed the fp32 kernels' register allocation.
__device__ __forceinline__ void store_logits(const MlpArgs& A, const f32x4 (&L)[STD_NOB], int pair, int g, bool live)
{
    if (live) {
        // the lane holds 4 consecutive logits per output block: one 16-byte store each (rows are
        // only 4-byte aligned when out_dim % 4 != 0; global dwordx4 stores allow that)
        float* o = A.out + (int64_t)pair * A.out_dim + 4 * g;
#pragma unroll
        for (int ob = 0; ob < STD_NOB; ++ob) {
            const int c0 = 16 * ob + 4 * g;
            if (c0 + 3 < A.out_dim) {
                *reinterpret_cast<f32x4u*>(o + 16 * ob) = L[ob];
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (c0 + r < A.out_dim) o[16 * ob + r] = L[ob][r];
            }
        }
    }
}
template <bool HEADS, bool SEL>
__device__ __forceinline__ void decode_block(const MlpArgs& A, const f32x4 (&L)[STD_NOB], f32x2 ut, f32x2 ur, unsigned row, bool live,
                                             int g, int lane, const float* lut)
{
    int k;
    // nocs/inference.py:187-188 (fp32, left to right); the owning lane stores its value
    if (!SEL) {   // (the second pass only needs the rotation / sign / scale heads: the centre was decoded in the first)
        {
            const float v[8] = {L[0][0], L[0][1], L[0][2], L[0][3], L[1][0], L[1][1], L[1][2], L[1][3]};
            if (sample_seg<8>(v, ut[0], g, lane, k) && live) at_off<float>(A.outputs, row * 8u) = lut[k];
        }
        {
            const float v[8] = {L[2][0], L[2][1], L[2][2], L[2][3], L[3][0], L[3][1], L[3][2], L[3][3]};
            if (sample_seg<8>(v, ut[1], g, lane, k) && live) at_off<float>(A.outputs, row * 8u + 4u) = lut[32 + k];
        }
    }
    if (HEADS) {
        const unsigned ho = row * 32u;
        {
            const float v[9] = {L[4][0], L[4][1], L[4][2], L[4][3], L[5][0], L[5][1], L[5][2], L[5][3], L[8][0]};
            if (sample_seg<9>(v, ur[0], g, lane, k) && live) at_off<float>(A.heads, ho) = lut[64 + k];
        }
        {
            const float v[9] = {L[6][0], L[6][1], L[6][2], L[6][3], L[7][0], L[7][1], L[7][2], L[7][3], L[8][1]};
            if (sample_seg<9>(v, ur[1], g, lane, k) && live) at_off<float>(A.heads, ho + 4u) = lut[64 + k];
        }
        // block 8, registers 2..3: aux_up aux_right | sx sy | sz - (dec_col)
        if (live && g < 2) { f32x2 w; w[0] = L[8][2]; w[1] = L[8][3]; at_off<f32x2>(A.heads, ho + 8u + 8u * g) = w; }
        if (live && g == 2) { f32x2 w; w[0] = L[8][2]; w[1] = 0.f; at_off<f32x2>(A.heads, ho + 24u) = w; }
    }
}

// The lane's share of one pair's layer-0 inputs: its 4 x 4 outputs of TA[a] and TB[b]
struct L0Gather { f32x4 ta[4], tb[4]; };
__device__ __forceinline__ L0Gather gather_l0(const MlpArgs& A, int ia, int ib, int g)
{
    L0Gather G;
    const unsigned oa = (unsigned)ia * (PROJ_COLS * 4u) + 16u * g, ob_ = (unsigned)ib * (PROJ_COLS * 4u) + 256u + 16u * g;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob) { G.ta[ob] = at_off<f32x4>(A.table, oa + 64u * ob); G.tb[ob] = at_off<f32x4>(A.table, ob_ + 64u * ob); }
    return G;
}

// The kernel's body for workgroup `wg` of the `n_wg` that share the pair list of `A` (pair_mlp.hip: pair_mlp_body; the same tile
// claim, the same software pipeline over tiles: indices two tiles ahead, points / normals and table gathers one tile ahead).
template <bool LOGITS, bool DECODE, bool HEADS, bool SEL>
__device__ __forceinline__ void pair_mlp_bf16_body(const MlpArgs& A, const int wg, const int n_wg)
{
    extern __shared__ __attribute__((aligned(16))) float W[];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(A.packed);
        f32x4* dst = reinterpret_cast<f32x4*>(W);
        // the decode variants take the final layer (weights and bias) from the copy whose output columns are in dec_col order
        for (int k = threadIdx.x; k < BF16_LDS / 4; k += MLP_THREADS) {
            int from = k;
            if (DECODE && k >= BOFF_WF / 4 && k < BOFF_B0B / 4) from = BOFF_WFD / 4 + (k - BOFF_WF / 4);
            if (DECODE && k >= BOFF_BF / 4) from = BOFF_BFD / 4 + (k - BOFF_BF / 4);
            dst[k] = src[from];
        }
    }
    float* lut = W + BF16_LDS;  // [0,32) mu, [32,64) nu, [64,100) theta: bin -> value, as in pair_mlp_body
    int* tile_ctr = reinterpret_cast<int*>(W + BF16_LDS + 112);
    if (threadIdx.x == 0) *tile_ctr = 0;
    if (DECODE && threadIdx.x < 100) {
        const int k = threadIdx.x;
        float v;
        if (k < 32) v = ((float)k / 31.0f * 2.0f) * A.vr0 - A.vr0;
        else if (k < 64) v = (float)(k - 32) / 31.0f * A.vr1;
        else v = (float)(k - 64) / 35.0f * (float)CPPF_PI;
        lut[k] = v;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    __builtin_assume(g >= 0 && g < 4);
    int Pn = (int)A.P;
    if (SEL) Pn = min(max(*A.n_sel, 0), Pn);
    const int n_tiles = (Pn + 15) / 16;
    // tiles are handed out per workgroup through an LDS counter (pair_mlp_body)
    const int per_wg = (n_tiles + n_wg - 1) / n_wg;
    const int wg_begin = wg * per_wg;
    const int wg_end = min(wg_begin + per_wg, n_tiles);
    auto claim = [&]() -> int {
        int v = 0;
        if (lane == 0) v = atomicAdd(tile_ctr, 1);
        return wg_begin + __builtin_amdgcn_readfirstlane(v);
    };
    int cur = claim();
    if (cur >= wg_end) return;
    int nxt = claim();

    // layer-0 accumulators of the tile about to run (fp32: acc[0..1] = fc1, acc[2..3] = fc0) and the pair indices of the one after
    f32x4 acc[4];
    int ia1, ib1;
    {
        int ia, ib;
        load_pair_idx<SEL>(A, cur * 16 + j, Pn, ia, ib);
        const L0Gather G = gather_l0(A, ia, ib, g);
        const float xp = ppf_from(ld3o(A.pc, ia), ld3o(A.pc, ib), ld3o(A.nrm, ia), ld3o(A.nrm, ib), g);
        const int nt = nxt < wg_end ? nxt : cur;   // (no next tile: reload this one, the values are never used)
        load_pair_idx<SEL>(A, nt * 16 + j, Pn, ia1, ib1);
        const f32x4 w = ldb4(W + BOFF_W0P + lane * 4);
#pragma unroll
        for (int ob = 0; ob < 4; ++ob) acc[ob] = mfma4(w[ob], xp, G.ta[ob] + G.tb[ob]);
    }

    for (;;) {
        const int tile = cur;
        asm volatile("" ::: "memory");   // (keeps the loop-invariant LDS weights from being hoisted into registers: pair_mlp_body)
        const int pair = tile * 16 + j;                      // slot of the launch
        const unsigned row = pair_row<SEL>(A, pair, Pn);     // row of the pair arrays

        // ---- next tile: points / normals in flight during the chain
        const f3 npa = ld3o(A.pc, ia1), npb = ld3o(A.pc, ib1), nna = ld3o(A.nrm, ia1), nnb = ld3o(A.nrm, ib1);
        f32x2 ut = {0.f, 0.f}, ur = {0.f, 0.f};
        if (DECODE) {
            const unsigned po = row * 8u;
            if (!SEL) ut = at_off<f32x2>(A.u_tr, po);
            if (HEADS) ur = at_off<f32x2>(A.u_rot, po);
        }

        // ---- layer 0: fc2 (32 -> 32) on bf(relu(fc1)), + fc0
        f32x4 x[2];
        {
            const bf16x8 a0 = bf8(relu4(acc[0]), relu4(acc[1]));
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
                x[ob] = mfma32b(ldw8(W + BOFF_W0B + (ob * 64 + lane) * 4), a0, ldb4(W + BOFF_B0B + 16 * ob + 4 * g)) + acc[2 + ob];
        }
        // ---- layer 1: 32 -> 32 -> 32, identity skip (the unrounded fp32 x)
        {
            const bf16x8 h = bf8(x[0], x[1]);
            f32x4 a1[2];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) a1[ob] = mfma32b(ldw8(W + BOFF_W1A + (ob * 64 + lane) * 4), h, ldb4(W + BOFF_B1A + 16 * ob + 4 * g));
            const bf16x8 a = bf8(relu4(a1[0]), relu4(a1[1]));
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
                x[ob] = mfma32b(ldw8(W + BOFF_W1B + (ob * 64 + lane) * 4), a, ldb4(W + BOFF_B1B + 16 * ob + 4 * g)) + x[ob];
        }
        // ---- next tile: PPF from the landed points, table gathers (consumed after layer 2), the indices of the tile after it
        const float xp = ppf_from(npa, npb, nna, nnb, g);
        const L0Gather G = gather_l0(A, ia1, ib1, g);
        const int nxt2 = claim();
        {
            const int nt = nxt2 < wg_end ? nxt2 : tile;
            load_pair_idx<SEL>(A, nt * 16 + j, Pn, ia1, ib1);
        }
        // ---- layer 2: fc1 | fc0 (32 -> 16 | 16) on bf(x), fc2 (16 -> 16) on bf(relu(fc1))
        bf16x4 zb;
        {
            const bf16x8 h = bf8(x[0], x[1]);
            const f32x4 a1 = mfma32b(ldw8(W + BOFF_W2 + lane * 4), h, ldb4(W + BOFF_B2 + 4 * g));
            const f32x4 s0 = mfma32b(ldw8(W + BOFF_W2 + (64 + lane) * 4), h, ldb4(W + BOFF_B2 + 16 + 4 * g));
            const f32x4 a2 = mfma16b(ldw4(W + BOFF_W2B + lane * 2), bf4(relu4(a1)), ldb4(W + BOFF_B2B + 4 * g));
            zb = bf4(a2 + s0);
        }
        // ---- layer 0 of the next tile (fp32) from the gathers that have been in flight since layer 1
        {
            const f32x4 w = ldb4(W + BOFF_W0P + lane * 4);
#pragma unroll
            for (int ob = 0; ob < 4; ++ob) acc[ob] = mfma4(w[ob], xp, G.ta[ob] + G.tb[ob]);
        }
        // ---- final 16 -> 144 (9 x 16) and the epilogue
        {
            // a decode without the rotation heads consumes only the two centre heads = output blocks 0..3 in dec_col order
            constexpr int NOB_USED = (DECODE && !HEADS) ? 4 : STD_NOB;
            f32x4 L[STD_NOB];
#pragma unroll
            for (int ob = 0; ob < STD_NOB; ++ob) L[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ob = 0; ob < NOB_USED; ++ob)
                L[ob] = mfma16b(ldw4(W + BOFF_WF + (ob * 64 + lane) * 2), zb, ldb4(W + BOFF_BF + 16 * ob + 4 * g));
            const bool live = pair < Pn;
            if (LOGITS) store_logits(A, L, pair, g, live);
            if (DECODE) decode_block<HEADS, SEL>(A, L, ut, ur, row, live, g, lane, lut);
        }
        cur = nxt;
        nxt = nxt2;
        if (cur >= wg_end) break;
    }
}

template <bool LOGITS, bool DECODE, bool HEADS>
__global__ __launch_bounds__(MLP_THREADS, MLP_WAVES_PER_SIMD) void pair_mlp_bf16_kernel(MlpArgs A)
{
    pair_mlp_bf16_body<LOGITS, DECODE, HEADS, false>(A, (int)blockIdx.x, (int)gridDim.x);
}

// Several pair lists in ONE launch: pair_mlp.hip's pair_mlp_batch_kernel with the bf16 body (same two mappings of workgroups to lists).
template <bool HEADS, bool SEL = false>
__global__ __launch_bounds__(MLP_THREADS, MLP_WAVES_PER_SIMD) void pair_mlp_bf16_batch_kernel(MlpBatch B)
{
    if (!SEL && B.per_xcd > 0) {
        const int x = (int)blockIdx.x & 7, r = (int)blockIdx.x >> 3;
        const int i = x / B.per_xcd;
        pair_mlp_bf16_body<false, true, HEADS, false>(B.item[i], r * B.per_xcd + x % B.per_xcd, ((int)gridDim.x >> 3) * B.per_xcd);
        return;
    }
    int i = 0;
    while (i + 1 < B.n && (int)blockIdx.x >= B.wg_begin[i + 1]) ++i;
    pair_mlp_bf16_body<false, true, HEADS, SEL>(B.item[i], (int)blockIdx.x - B.wg_begin[i], B.wg_begin[i + 1] - B.wg_begin[i]);
}

// ----------------------------------------------------------------------------- entry points
// the bf16 kernels as a PairVariant: everything else on the host side is pair_mlp.hip's shared code (pair_mlp_common.h)
static int launch_logits(const MlpArgs& A, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((pair_mlp_bf16_kernel<true, false, false>), dim3(mlp_grid(A.P)), dim3(MLP_THREADS), lds, st, A);
    CPPF_CHECK_LAUNCH();
    return 0;
}
static int launch_batch(const MlpBatch& B, bool heads, bool sel, unsigned grid, size_t lds, hipStream_t st)
{
    if (!sel && heads) hipLaunchKernelGGL((pair_mlp_bf16_batch_kernel<true>), dim3(grid), dim3(MLP_THREADS), lds, st, B);
    else if (!sel) hipLaunchKernelGGL((pair_mlp_bf16_batch_kernel<false>), dim3(grid), dim3(MLP_THREADS), lds, st, B);
    else hipLaunchKernelGGL((pair_mlp_bf16_batch_kernel<true, true>), dim3(grid), dim3(MLP_THREADS), lds, st, B);
    CPPF_CHECK_LAUNCH();
    return 0;
}
static const PairVariant PAIR_BF16 = {(BF16_LDS + 128) * sizeof(float), launch_logits, launch_batch, /* skip_empty */ true};

extern "C" int cppf_pair_mlp_bf16_forward(const float* pc, const float* nrm, const float* feat, const void* idxs, int idx_is_i64,
                                          const void* packed, int64_t N, int F, const int* dims, int n_res, int64_t P, int out_dim,
                                          float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (P < 0 || !dims) return CPPF_EINVAL;
    if (!is_std(F, dims, n_res, out_dim)) return CPPF_EUNSUPPORTED;   // (no generic bf16 kernel)
    if (P == 0) return 0;
    if (!pc || !nrm || !feat || !idxs || !packed || !out) return CPPF_EINVAL;
    MlpArgs A = {};
    A.pc = pc; A.nrm = nrm; A.feat = feat; A.idxs = idxs; A.packed = static_cast<const float*>(packed); A.out = out; A.P = P;
    A.out_dim = out_dim; A.idx64 = idx_is_i64;
    return pair_std_forward(PAIR_BF16, A, N, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int cppf_pair_mlp_bf16_decode_batch(int n_items, const CppfPairMlpItem* items, int F, const int* dims, int n_res, int out_dim,
                                               int tr_bins, int rot_bins, void* stream)
{
    return pair_decode_batch(PAIR_BF16, n_items, items, F, dims, n_res, out_dim, tr_bins, rot_bins, (hipStream_t)stream);
}
extern "C" int cppf_pair_mlp_bf16_decode_sel_batch(int n_items, const CppfPairMlpItem* items, int F, const int* dims, int n_res,
                                                   int out_dim, int tr_bins, int rot_bins, void* stream)
{
    return pair_decode_sel_batch(PAIR_BF16, n_items, items, F, dims, n_res, out_dim, tr_bins, rot_bins, (hipStream_t)stream);
}
