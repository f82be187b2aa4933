// What the fp32 pair encoder (pair_mlp.hip) and the bf16 one (pair_mlp_bf16.hip) share: the argument blocks of their kernels, the PPF
// construction, the addressing helpers of the tile loop, the two in-register samplers, the decode of the heads, the launch
// geometry and the host path of the entry points.  The device functions are all force-inlined: each file instantiates its own
// kernels, and the host side of both goes through pair_mlp.hip's pair_std_forward / pair_decode_batch / pair_decode_sel_batch with a
// PairVariant that names the kernels to launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cppf.h"
#include "cppf_math.h"
#include "pair_layout.h"   // packed image: offsets, khid, dec_col, std_pack_elem

using namespace cppf;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));  // 16-byte access at 4-byte alignment

#define CPPF_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t e__ = hipGetLastError();         \
        if (e__ != hipSuccess) return (int)e__;     \
    } while (0)

static bool is_std(int F, const int* dims, int n_res, int out_dim)
{
    return F == STD_F && n_res == 3 && dims[0] == 84 && dims[1] == 32 && dims[2] == 32 && dims[3] == 16 &&
           out_dim >= 1 && out_dim <= 16 * STD_NOB;
}

#define MLP_THREADS 1024
#define MLP_WAVES_PER_SIMD 4
#define PB 1  // 16-pair blocks per wave tile

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// max(v, 0) as ONE v_max_f32.  On a value the compiler cannot prove to be no signalling NaN (an MFMA result, a crossbar
// exchange) fmaxf / `v > 0 ? v : 0` is preceded by a canonicalising v_max_f32 v, v -- 20 extra instructions per tile on the
// pipe the MFMAs share -- unless the file is built with -fno-honor-nans (Makefile).  Not inline assembly: the compiler
// does not count an asm statement as a VALU instruction when it places the wait states an MFMA result needs before its
// first VALU reader, so an asm v_max_f32 on an accumulator reads it early (seen: run-to-run differences in the logits).
__device__ __forceinline__ float relu1(float v) { return fmaxf(v, 0.f); }
__device__ __forceinline__ f32x4 relu4(f32x4 v)
{
    f32x4 r;
    r[0] = relu1(v[0]); r[1] = relu1(v[1]); r[2] = relu1(v[2]); r[3] = relu1(v[3]);
    return r;
}
__device__ __forceinline__ f32x4 ldb4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- decode helpers (semantics: oracle/cppf_oracle.c:orc_sample_bin) --------------------------
// Logit 16*R + 4*g + r of the lane's pair lives in L[R][r] of lane group g = lane >> 4: one "chunk"
// of 4 consecutive logits per lane per MFMA output block ("row") R.  Cross-lane traffic inside the
// 4 lanes of a pair goes through the LDS crossbar (ds_swizzle / ds_bpermute: no LDS memory, and no VALU
// issue slots -- a v_permlane*_swap exchange costs 2 moves + swap (2 slots) + select = 5 slots on the pipe
// the fp32 MFMAs also need; measured 3 % faster, profiles/microbench/valu_bench.hip).
__device__ __forceinline__ unsigned xor16u(unsigned v, int lane)
{
    (void)lane;
    return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x401f);  // bit mode: and 0x1f, or 0, xor 0x10
}
__device__ __forceinline__ unsigned xor32u(unsigned v, int lane)
{
    return (unsigned)__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, (int)v);
}
__device__ __forceinline__ float xor16f(float v, int lane) { return __uint_as_float(xor16u(__float_as_uint(v), lane)); }
__device__ __forceinline__ float xor32f(float v, int lane) { return __uint_as_float(xor32u(__float_as_uint(v), lane)); }

// One head whose NL consecutive bins NL*g .. NL*g + NL-1 sit in v[] of lane group g (dec_col layout).  Semantics:
// oracle/cppf_oracle.c:orc_sample_bin.  Returns true in exactly one of the pair's 4 lanes -- the one that owns
// the sampled bin -- with the bin index.
template <int NL>
__device__ __forceinline__ bool sample_seg(const float (&v)[NL], float u, int g, int lane, int& bin)
{
    static_assert(NL == 8 || NL == 9, "the draw below searches 7 running sums + at most one more");
    float m = v[0];
#pragma unroll
    for (int k = 1; k < NL; ++k) m = fmaxf(m, v[k]);   // (v_max3_f32 pairs; no canonicalising moves under -fno-honor-nans)
    float mall = fmaxf(m, xor16f(m, lane));
    mall = fmaxf(mall, xor32f(mall, lane));
    // softmax weights 2^(l log2e - max log2e): the max subtraction rides on the exponent's fma (cppf_math.h:det_exp2w)
    const float c = -(mall * CPPF_LOG2E);
    float e[NL];
    // (scalar instructions on purpose: beside the fp32 MFMAs, which run on the same datapath, a v_pk_fma_f32 costs as much as
    //  the two v_fma_f32 it replaces or more -- packed exponentials and the compiler's SLP packing measured 2.5-3 % slower,
    //  profiles/r2_pair_mlp_phases.txt; the Makefile passes -fno-slp-vectorize)
#pragma unroll
    for (int k = 0; k < NL; ++k) e[k] = det_exp2w(v[k], c);
    // running sums of the lane's segment: the last one is the segment total, and the draw compares them with the
    // threshold moved into the segment (t - off) -- one chain of NL - 1 additions serves both
    float b[NL];
    b[0] = e[0];
#pragma unroll
    for (int k = 1; k < NL; ++k) b[k] = b[k - 1] + e[k];
    const float T = b[NL - 1];
    const float Tp = xor16f(T, lane);           // the other lane of my half
    const float half = T + Tp;                  // T0 + T1 in lanes g = 0,1; T2 + T3 in lanes g = 2,3 (a+b == b+a)
    const float oth = xor32f(half, lane);
    const float off = ((g & 2) ? oth : 0.f) + ((g & 1) ? Tp : 0.f);
    const float t = u * ((g & 2) ? oth + half : half + oth) - off;   // u * ((T0 + T1) + (T2 + T3)) - off_g
    // first k with b[k] > t, NL - 1 when there is none.  The weights are >= 0, so the running sums never decrease and the
    // oracle's scan in k order finds what a bisection finds: three compares over b[0..6] instead of seven (+ one for NL = 9).
    const bool c1 = b[3] > t;
    const bool c2 = (c1 ? b[1] : b[5]) > t;
    const float lo = c2 ? b[0] : b[2], hi = c2 ? b[4] : b[6];
    const bool c3 = (c1 ? lo : hi) > t;
    int kk = (c1 ? 0 : 4) + (c2 ? 0 : 2) + (c3 ? 0 : 1);
    if (NL == 9) kk = b[7] > t ? kk : 8;
    // the pair's first segment with a hit owns the draw (none: the last bin, which lane 3's search has found by itself).
    // The ballot is wave-uniform, so "first of the four lanes j, j + 16, j + 32, j + 48" is scalar arithmetic on its four
    // 16-bit quarters, and the owner's predicate goes straight back into a lane mask: no VALU instruction after the compare
    // (the per-lane shift / and / find-first-bit form took thirteen).
    const unsigned long long hm = __ballot(b[NL - 1] > t);
    const unsigned h0 = (unsigned)hm & 0xffffu, h1 = (unsigned)(hm >> 16) & 0xffffu, h2 = (unsigned)(hm >> 32) & 0xffffu;
    const unsigned o1 = h1 & ~h0, o2 = h2 & ~(h0 | h1), o3 = ~(h0 | h1 | h2) & 0xffffu;
    const unsigned long long own = (unsigned long long)(h0 | (o1 << 16)) | ((unsigned long long)(o2 | (o3 << 16)) << 32);
    bool owner = __builtin_amdgcn_inverse_ballot_w64(own);
    bin = NL * g + kk;
    if (__any(u < 0.f)) {  // arg-max mode (rare, wave-uniform test so the common path really skips it)
        asm volatile("" ::: "memory");
        int ak = 64;   // (position inside the segment first, its base added once: `am = NL * g + k` per k made the compiler keep
#pragma unroll     //  NL loop-invariant registers per head for this rarely taken path -- the all-heads variant spilled)
        for (int k = NL - 1; k >= 0; --k)
            if (v[k] == mall) ak = k;
        const int am = NL * g + ak;   // a lane without the maximum: >= 64, above every bin
        int best = min(am, (int)xor16u((unsigned)am, lane));
        best = min(best, (int)xor32u((unsigned)best, lane));
        if (u < 0.f) { bin = best; owner = am == best; }
    }
    return owner;
}

struct MlpArgs {
    const float* pc;
    const float* nrm;
    const float* feat;
    const void* idxs;
    const float* packed;
    const float* u_tr;
    const float* u_rot;
    const float* table;  // [N][128] per-point layer-0 projections (point_proj_kernel)
    float* out;      // logits [P,out_dim]   (LOGITS)
    float* outputs;  // [P,2]                (DECODE)
    float* heads;    // [P,8] or null        (DECODE)
    int64_t P;
    int out_dim;
    int idx64;
    float vr0, vr1;
    // SEL variant (second MLP pass of nocs/inference.py:236 on the pairs that survived the back-vote): slot i of the launch
    // works on pair sel[i], i < min(*n_sel, P); everything per pair (indices, uniforms, results) stays at the pair's own row
    const int32_t* sel;
    const int32_t* n_sel;
};

// Addresses inside the tile loop are a uniform base (SGPR pair) + an unsigned 32-bit byte offset (one VGPR): the
// `global_load v, v_off, s[base]` form.  64-bit pointer arithmetic per lane (v_lshl_add_u64, v_lshlrev_b64 ...) was ~50 VALU
// per tile on the pipe the fp32 MFMAs share.  Hence the limits of the MFMA path: N < 2^23 points, P < 2^27 pairs (std_table, item_limits).
template <typename T>
__device__ __forceinline__ const T& at_off(const void* base, unsigned byte_off)
{
    return *reinterpret_cast<const T*>(static_cast<const char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ T& at_off(void* base, unsigned byte_off)
{
    return *reinterpret_cast<T*>(static_cast<char*>(base) + byte_off);
}
__device__ __forceinline__ f3 ld3o(const float* __restrict__ base, int i)
{
    const unsigned o = __umul24((unsigned)i, 12u);   // (N < 2^23 on this path: the full-rate 24-bit multiply; v_mul_lo_u32 takes four issue slots)
    // (the +4 / +8 ride on the uniform base, i.e. in the instruction's immediate offset: added to the 32-bit lane offset they are
    //  two v_add_u32 per index, because unsigned wrap-around has to be preserved)
    return {at_off<float>(base, o), at_off<float>(base + 1, o), at_off<float>(base + 2, o)};
}

// slot of the launch -> row of the pair arrays (identity unless SEL)
// (slots, tiles and pair counts are 32-bit inside the kernel -- P < 2^27, item_limits -- : 64-bit compares and selects were a
//  dozen instructions per tile)
template <bool SEL>
__device__ __forceinline__ unsigned pair_row(const MlpArgs& A, int slot, int Pn)
{
    const unsigned s = (unsigned)min(slot, Pn - 1);
    return SEL ? (unsigned)at_off<int>(A.sel, s * 4u) : s;
}

template <bool SEL>
__device__ __forceinline__ void load_pair_idx(const MlpArgs& A, int slot, int Pn, int& ia, int& ib)
{
    // two 4-byte loads of the low words whatever the index width: an i32 / i64 branch around the loads ends in a
    // wait for ALL outstanding loads (the gathers of the next tile that are in flight at this point)
    const unsigned p = pair_row<SEL>(A, slot, Pn);
    const unsigned o = p * (A.idx64 ? 16u : 8u);
    ia = at_off<int>(A.idxs, o);
    ib = at_off<int>(static_cast<const char*>(A.idxs) + (A.idx64 ? 8 : 4), o);   // (second column through the uniform base)
}

// PPF of one pair from already loaded points/normals (models/model.py:118-129); component `g`.
__device__ __forceinline__ float ppf_from(f3 pa, f3 pb, f3 na, f3 nb, int g)
{
    const f3 xy = sub3(pa, pb);
    const float d = sqrt_rn((xy.x * xy.x + xy.y * xy.y) + xy.z * xy.z);
    const float den = d + 1e-7f;                       // fp32 add (torch), unlike the vote kernels
    // three IEEE divisions by one denominator (den in [1e-7, ~2], |xy| <= d: no rescaling or fix-up would apply): div_by()
    const float rden = refined_rcp(den);
    const f3 u = {div_by(xy.x, den, rden), div_by(xy.y, den, rden), div_by(xy.z, den, rden)};
    const float p0 = (na.x * u.x + na.y * u.y) + na.z * u.z;
    const float p1 = (nb.x * u.x + nb.y * u.y) + nb.z * u.z;
    const float p2 = (na.x * nb.x + na.y * nb.y) + na.z * nb.z;
    // 4-way select by lane group: g = lane >> 4, so "g == k" is a constant lane mask -- three v_cndmask on scalar masks
    // (the and / or form on per-lane masks took eleven; a ?: chain on g itself becomes divergent branches that split the
    // MFMA schedule)
    (void)g;
    const bool g0 = __builtin_amdgcn_inverse_ballot_w64(0x000000000000ffffull), g1 = __builtin_amdgcn_inverse_ballot_w64(0x00000000ffff0000ull),
               g2 = __builtin_amdgcn_inverse_ballot_w64(0x0000ffff00000000ull);
    const float s23 = g2 ? p2 : d, s123 = g1 ? p1 : s23;
    return g0 ? p0 : s123;
}

#define PROJ_PPB 8
// the projections of several clouds in one launch (cppf_pair_mlp_decode_batch): cloud blockIdx.y; as wide as the largest needs
struct ProjBatch { const float* feat[8]; const float* packed[8]; float* table[8]; int64_t N[8]; };

#define MLP_BATCH_MAX 8
struct MlpBatch {
    MlpArgs item[MLP_BATCH_MAX];
    int wg_begin[MLP_BATCH_MAX + 1];
    int n;
    int per_xcd;   // > 0: lists of (nearly) equal length, 8 % n == 0: list i on XCDs [i per_xcd, (i + 1) per_xcd) -- see below
};
static_assert(sizeof(ProjBatch) <= 4096, "ProjBatch travels by value: kernel arguments are limited to 4 KB");
static_assert(sizeof(MlpBatch) <= 4096, "MlpBatch travels by value: kernel arguments are limited to 4 KB");

static int mlp_grid(int64_t P)
{
    const int64_t tiles = (P + 16 * PB - 1) / (16 * PB);
    int64_t nb = (tiles + MLP_THREADS / 64 - 1) / (MLP_THREADS / 64);
    const int64_t resident = 256 * (MLP_WAVES_PER_SIMD * 4 / (MLP_THREADS / 64));  // workgroups the chip holds at once
    if (nb > resident) nb = resident;
    if (nb < 1) nb = 1;
    return (int)nb;
}

// ---- host path.  What differs between the two encoders once a call is known to be for the standard architecture: the kernels (each
// file launches its own) and one rule.  Everything else -- the item contract, the MlpArgs / ProjBatch fills, the per-point tables,
// the launch geometry, the survivor capacity, the 2^23 / 2^27 limits -- is the three bodies below, defined once in pair_mlp.hip.
struct PairVariant {
    size_t lds_bytes;   // dynamic LDS of the variant's pair kernels
    // the logits kernel on mlp_grid(A.P) workgroups
    int (*launch_logits)(const MlpArgs& A, size_t lds, hipStream_t st);
    // the batch kernel <heads, sel> on `grid` workgroups (sel: the second pass, always with heads), with whatever function
    // attribute the kernel needs for `lds`
    int (*launch_batch)(const MlpBatch& B, bool heads, bool sel, unsigned grid, size_t lds, hipStream_t st);
    // a list with n_pairs == 0 in the first-pass batch: true = skipped (0 when no list is left), false = CPPF_EINVAL
    bool skip_empty;
};
#define PAIR_HOST __attribute__((visibility("hidden")))
// logits of one list: the checks of the MFMA path (N, the limits, the workspace), the per-point table, V.launch_logits.  The caller
// has checked the architecture and the pointers and filled A (all but A.table).
PAIR_HOST int pair_std_forward(const PairVariant& V, MlpArgs& A, int64_t N, void* workspace, size_t workspace_bytes, hipStream_t st);
// cppf_pair_mlp[_bf16]_decode_batch and _decode_sel_batch, whole
PAIR_HOST int pair_decode_batch(const PairVariant& V, int n_items, const CppfPairMlpItem* items, int F, const int* dims, int n_res,
                                int out_dim, int tr_bins, int rot_bins, hipStream_t st);
PAIR_HOST int pair_decode_sel_batch(const PairVariant& V, int n_items, const CppfPairMlpItem* items, int F, const int* dims, int n_res,
                                    int out_dim, int tr_bins, int rot_bins, hipStream_t st);
