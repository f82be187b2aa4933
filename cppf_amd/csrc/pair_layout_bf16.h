// Packed weight image of the bf16 pair encoder (pair_mlp_bf16.hip): the standard architecture (F = 40, ppffcs = [84, 32, 32, 16]) with
// layer 0 and every bias in fp32 and the weights of every later layer rounded to bf16 (round to nearest even).  Offsets are in FLOATS
// (4-byte words; a bf16 section holds two weights per word).  As for the fp32 image (pair_layout.h) ONE function, bf16_pack_word(),
// says what every word holds; the host pack and the device pack both evaluate it.
//
// MFMA operand convention.  Lane l = (j = l & 15, g = l >> 4).
//   v_mfma_f32_16x16x32_bf16: the A operand is 8 bf16 per lane, element jj = A[row j][k-slot 8g + jj]; the B operand a lane supplies
//     after a 32-wide layer is its 8 accumulator values (block ob = jj >> 2, register r = jj & 3) = features 16*(jj >> 2) + 4g + (jj & 3):
//     k32(g, jj) below, the bf16 counterpart of khid().
//   v_mfma_f32_16x16x16_bf16: 4 bf16 per lane, element i = A[row j][k = 4g + i] -- the lane's 4 accumulator values of a 16-wide layer
//     are already its 4 k-slots, natural order.
// The layer-0 section (per-point projection weights, fc1 | fc0 bias) sits at the fp32 image's own offsets OFF_WPT / OFF_BPT, so the
// point_proj kernels of pair_mlp.hip read either image.
#pragma once
#include "pair_layout.h"

#define BOFF_W0P 0                         // f32  [64][4]      PPF k-step of layer 0, as OFF_W0P
#define BOFF_W0B (BOFF_W0P + 64 * 4)       // bf16 [2][64][8]   layer 0 fc2: block ob, lane, k-slot
#define BOFF_W1A (BOFF_W0B + 2 * 64 * 4)   // bf16 [2][64][8]   layer 1 fc1
#define BOFF_W1B (BOFF_W1A + 2 * 64 * 4)   // bf16 [2][64][8]   layer 1 fc2
#define BOFF_W2 (BOFF_W1B + 2 * 64 * 4)    // bf16 [2][64][8]   block 0 = layer 2 fc1 (16 outputs), block 1 = layer 2 fc0
#define BOFF_W2B (BOFF_W2 + 2 * 64 * 4)    // bf16 [64][4]      layer 2 fc2 (K = 16 form)
#define BOFF_WF (BOFF_W2B + 64 * 2)        // bf16 [9][64][4]   final (K = 16 form), natural output columns
#define BOFF_B0B (BOFF_WF + STD_NOB * 64 * 2)  // f32 biases in natural output order, as OFF_B0B ..
#define BOFF_B1A (BOFF_B0B + 32)
#define BOFF_B1B (BOFF_B1A + 32)
#define BOFF_B2 (BOFF_B1B + 32)
#define BOFF_B2B (BOFF_B2 + 32)
#define BOFF_BF (BOFF_B2B + 16)
#define BF16_LDS (BOFF_BF + 144)           // 3 872 words = 15 488 B live in LDS
#define BOFF_WFD BF16_LDS                  // bf16 [9][64][4]   final with the output columns in DECODE order (dec_col)
#define BOFF_BFD (BOFF_WFD + STD_NOB * 64 * 2)  // f32 [144]    its bias, slot order
#define BOFF_WPT OFF_WPT                   // f32  [40][128]    = the fp32 image's section, same offset
#define BOFF_BPT OFF_BPT                   // f32  [64]
#define BF16_PACKED (OFF_BPT + 64)         // 13 152 words = 52 608 B
static_assert(BOFF_BFD + 144 <= BOFF_WPT, "the bf16 sections end before the shared layer-0 section");

static CPPF_HD inline int k32(int g, int jj) { return 16 * (jj >> 2) + 4 * g + (jj & 3); }

// fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32's rounding; inputs are finite weights)
static CPPF_HD inline uint32_t bf16_bits(float f)
{
    union { float f; uint32_t u; } v;
    v.f = f;
    return (v.u + 0x7fffu + ((v.u >> 16) & 1u)) >> 16;
}
static CPPF_HD inline uint32_t bf16_pair(float lo, float hi) { return bf16_bits(lo) | (bf16_bits(hi) << 16); }
static CPPF_HD inline uint32_t f32_word(float f)
{
    union { float f; uint32_t u; } v;
    v.f = f;
    return v.u;
}

// Word `idx` of the image; params / offs as std_pack_elem.
static CPPF_HD inline uint32_t bf16_pack_word(int idx, const float* params, const int64_t* offs, int out_dim)
{
    const float *w1_0 = params + offs[0], *b1_0 = params + offs[1], *w2_0 = params + offs[2], *b2_0 = params + offs[3];
    const float *w0_0 = params + offs[4], *b0_0 = params + offs[5];
    const float *w1_1 = params + offs[6], *b1_1 = params + offs[7], *w2_1 = params + offs[8], *b2_1 = params + offs[9];
    const float *w1_2 = params + offs[12], *b1_2 = params + offs[13], *w2_2 = params + offs[14], *b2_2 = params + offs[15];
    const float *w0_2 = params + offs[16], *b0_2 = params + offs[17];
    const float *wf = params + offs[18], *bf = params + offs[19];
    if (idx < BOFF_W0B) {                      // [64][4] f32, as std_pack_elem
        const int l = idx >> 2, ob = idx & 3;
        const int o = 16 * (ob & 1) + (l & 15), k = 80 + (l >> 4);
        return f32_word((ob < 2 ? w1_0 : w0_0)[o * 84 + k]);
    }
    if (idx < BOFF_W2B) {                      // four [2][64][8] bf16 blocks: word = slots 2q, 2q + 1 of (ob, lane)
        const int which = (idx - BOFF_W0B) / 512, i = (idx - BOFF_W0B) % 512;
        const int ob = i >> 8, l = (i >> 2) & 63, q = i & 3, g = l >> 4;
        const float* w = which == 0 ? w2_0 : (which == 1 ? w1_1 : (which == 2 ? w2_1 : (ob == 0 ? w1_2 : w0_2)));
        const int o = (which == 3 ? 0 : 16 * ob) + (l & 15);
        return bf16_pair(w[o * 32 + k32(g, 2 * q)], w[o * 32 + k32(g, 2 * q + 1)]);
    }
    if (idx < BOFF_WF) {                       // [64][4] bf16
        const int i = idx - BOFF_W2B, l = i >> 1, q = i & 1, k = 4 * (l >> 4) + 2 * q;
        return bf16_pair(w2_2[(l & 15) * 16 + k], w2_2[(l & 15) * 16 + k + 1]);
    }
    if (idx < BOFF_B0B) {                      // [9][64][4] bf16, natural columns
        const int i = idx - BOFF_WF, ob = i >> 7, l = (i >> 1) & 63, q = i & 1, k = 4 * (l >> 4) + 2 * q;
        const int o = 16 * ob + (l & 15);
        return o < out_dim ? bf16_pair(wf[o * 16 + k], wf[o * 16 + k + 1]) : 0u;
    }
    if (idx < BOFF_B1A) return f32_word(b2_0[idx - BOFF_B0B]);
    if (idx < BOFF_B1B) return f32_word(b1_1[idx - BOFF_B1A]);
    if (idx < BOFF_B2) return f32_word(b2_1[idx - BOFF_B1B]);
    if (idx < BOFF_B2B) { const int o = idx - BOFF_B2; return f32_word(o < 16 ? b1_2[o] : b0_2[o - 16]); }
    if (idx < BOFF_BF) return f32_word(b2_2[idx - BOFF_B2B]);
    if (idx < BOFF_WFD) { const int o = idx - BOFF_BF; return o < out_dim ? f32_word(bf[o]) : 0u; }
    if (idx < BOFF_BFD) {                      // [9][64][4] bf16, decode column order
        if (out_dim != 141) return 0u;
        const int i = idx - BOFF_WFD, ob = i >> 7, l = (i >> 1) & 63, q = i & 1, k = 4 * (l >> 4) + 2 * q;
        const int m = l & 15, c = dec_col(ob, m >> 2, m & 3);
        return c >= 0 ? bf16_pair(wf[c * 16 + k], wf[c * 16 + k + 1]) : 0u;
    }
    if (idx < BOFF_BFD + 144) {
        if (out_dim != 141) return 0u;
        const int i = idx - BOFF_BFD, c = dec_col(i >> 4, (i & 15) >> 2, i & 3);
        return c >= 0 ? f32_word(bf[c]) : 0u;
    }
    if (idx < BOFF_WPT) return 0u;             // (unused words between the bf16 sections and the shared layer-0 section)
    if (idx < BOFF_BPT) {                      // [40][128] f32, as std_pack_elem
        const int i = idx - BOFF_WPT, k = i >> 7, r = i & 127, oc = r & 63;
        const float* w = oc < 32 ? w1_0 + oc * 84 : w0_0 + (oc - 32) * 84;
        return f32_word(w[(r < 64 ? 0 : 40) + k]);
    }
    { const int o = idx - BOFF_BPT; return f32_word(o < 32 ? b1_0[o] : b0_0[o - 32]); }
}
