// Weight image and MFMA helpers of the bf16 point encoder (sprin_bf16.hip): the kernel-MLP of the standard SPRIN layer
// (6 -> 32 -> 64 -> 32 -> 32 -> 32, sprin_layout.h) with layer 1 and every bias / gamma / beta vector in fp32 and the weights of
// layers 2..5 rounded to bf16 (round to nearest even).  Offsets are in 4-byte WORDS; a bf16 section holds two weights per word.
// ONE function, sp_bf16_image_word(), says what every word holds; the host pack and the device pack both evaluate it.
//
// v_mfma_f32_16x16x32_bf16, transposed as in sprin_layout.h: D[out][row] = W[out][k] * X^T[k][row], lane l = (j = l & 15, g = l >> 4).
//   A operand: 8 bf16 per lane, element e = W[16*ob + j][k-slot (g, e)], one 16-byte LDS read per MFMA.
//   B operand: the lane's own 8 activations of row j.  After a layer the lane holds outputs 16*ob + 4g + r of its row, so with
//              (ob, r) = (2h + (e >> 2), e & 3) k-slot (g, e) of the 32-input half h is input  32h + 16*(e >> 2) + 4g + (e & 3)
//              = sp_k32(h, g, e): the layers chain with no lane movement and no LDS, as the fp32 ones do through sp_khid().
//   D: f32x4 = outputs 16*ob + 4g + r of row j, fp32, seeded with the bias.
#pragma once
#include "sprin_layout.h"

namespace sprin {

constexpr int SPB_L1 = 0;                          // f32  [2 ob][2 s][64]         = the fp32 image's SPW_L1 section, word for word
constexpr int SPB_L2 = SPB_L1 + 2 * 2 * 64;        // bf16 [4 ob][1 h][64 lanes][8]
constexpr int SPB_L3 = SPB_L2 + 4 * 1 * 64 * 4;    // bf16 [2 ob][2 h][64 lanes][8]
constexpr int SPB_L4 = SPB_L3 + 2 * 2 * 64 * 4;    // bf16 [2 ob][1 h][64 lanes][8]
constexpr int SPB_L5 = SPB_L4 + 2 * 1 * 64 * 4;    // bf16 [2 ob][1 h][64 lanes][8]
constexpr int SPB_VEC = SPB_L5 + 2 * 1 * 64 * 4;   // f32  b1 g1 be1 b2 g2 be2 b3 g3 be3 b4 g4 be4 b5 = the SPW_VEC section
constexpr int SPB_B1 = SPB_VEC, SPB_B2 = SPB_B1 + 96, SPB_B3 = SPB_B2 + 192, SPB_B4 = SPB_B3 + 96, SPB_B5 = SPB_B4 + 96;
constexpr int SPB_WORDS = SPB_B5 + 32;             // 3 840 words = 15 KB (6 144 bf16 weights in 12 KB against 24 KB of fp32)
static_assert(SPB_L2 == SPW_L2 && SPB_WORDS % 4 == 0 && SPB_L2 % 4 == 0 && SPB_VEC % 4 == 0, "16-byte sections");

__host__ __device__ inline int sp_k32(int h, int g, int e) { return 32 * h + 16 * (e >> 2) + 4 * g + (e & 3); }

// fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32's rounding; inputs are finite weights)
__host__ __device__ inline uint32_t sp_bf16_bits(float f)
{
    union { float f; uint32_t u; } v;
    v.f = f;
    return (v.u + 0x7fffu + ((v.u >> 16) & 1u)) >> 16;
}
__host__ __device__ inline uint32_t sp_f32_word(float f)
{
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}

// word `idx` of one layer's bf16 image from the layer's natural parameters
__host__ __device__ inline uint32_t sp_bf16_image_word(int idx, const float* __restrict__ q)
{
    if (idx < SPB_L2) return sp_f32_word(sp_image_elem(SPW_L1 + idx, q));
    if (idx >= SPB_VEC) return sp_f32_word(sp_image_elem(SPW_VEC + (idx - SPB_VEC), q));
    const int L = idx < SPB_L3 ? 0 : (idx < SPB_L4 ? 1 : (idx < SPB_L5 ? 2 : 3));
    const int off = L == 0 ? SPB_L2 : (L == 1 ? SPB_L3 : (L == 2 ? SPB_L4 : SPB_L5));
    const int nat = L == 0 ? NAT_W2 : (L == 1 ? NAT_W3 : (L == 2 ? NAT_W4 : NAT_W5));
    const int n_in = L == 1 ? 64 : 32, NH = n_in / 32;
    const int i = idx - off, blk = i >> 8, ln = (i >> 2) & 63, e = 2 * (i & 3);   // word = k-slots e, e + 1 of (ob, h, lane)
    const int ob = blk / NH, h = blk % NH, g = ln >> 4;
    const float* w = q + nat + (16 * ob + (ln & 15)) * n_in;
    return sp_bf16_bits(w[sp_k32(h, g, e)]) | (sp_bf16_bits(w[sp_k32(h, g, e + 1)]) << 16);
}

typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));
typedef float sp_f32x8 __attribute__((ext_vector_type(8)));

// bf() of the lane's 8 values of one 32-input half: v_cvt_pk_bf16_f32, two values per instruction
__device__ __forceinline__ sp_bf16x8 sp_bf8(f32x4 lo, f32x4 hi)
{
    sp_f32x8 v;
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
    return __builtin_convertvector(v, sp_bf16x8);
}

// One bf16 layer for TWO row blocks (the counterpart of sp_mfma_layer2): inputs 32*NH per row, already LayerNormed and
// rectified in fp32 and rounded here; outputs 16*NOB in fp32 on the bias seed.  Every 16-byte weight read feeds both blocks.
template <int NH, int NOB>
__device__ __forceinline__ void sp_bf16_layer2(const float* __restrict__ Wb, const float* __restrict__ bias, const f32x4 (&xa)[2 * NH],
                                               const f32x4 (&xb)[2 * NH], f32x4 (&ya)[NOB], f32x4 (&yb)[NOB], int lane, int g)
{
    sp_bf16x8 pa[NH], pb[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) { pa[h] = sp_bf8(xa[2 * h], xa[2 * h + 1]); pb[h] = sp_bf8(xb[2 * h], xb[2 * h + 1]); }
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) { ya[ob] = *reinterpret_cast<const f32x4*>(bias + 16 * ob + 4 * g); yb[ob] = ya[ob]; }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            const sp_bf16x8 w = *reinterpret_cast<const sp_bf16x8*>(Wb + ((ob * NH + h) * 64 + lane) * 4);
            ya[ob] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, pa[h], ya[ob], 0, 0, 0);
            yb[ob] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, pb[h], yb[ob], 0, 0, 0);
        }
    }
}

}  // namespace sprin
