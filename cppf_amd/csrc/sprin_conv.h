// The SPRIN convolution's device body and launch description, shared by the fp32 kernels (sprin.hip) and the bf16 kernels
// (sprin_bf16.hip): gather, rifeat, the kernel-MLP, the rank contraction, the outnet with its LayerNorm, GlobalInfoProp's linear and
// the workgroup maxima, the `n_dev` handling.  The two precisions differ in the kernel-MLP alone (template parameter BF16: the
// fp32 instantiation is the text sprin.hip held before the split, the bf16 one swaps layers 2..5 for sp_bf16_layer2); each file
// instantiates its own kernels, and the host side of both goes through sprin.hip's cppf_internal_sprin_forward / _batch with an
// SpVariant that names the kernels to launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cppf.h"
#include "cppf_math.h"
#include "sprin_layout.h"
#include "sprin_layout_bf16.h"

namespace sprin {

using namespace cppf;

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

constexpr int SP_BATCH_MAX = 8;

__host__ __device__ constexpr int sp_per_wave(int n_in) { return 16 * SP_KSTRIDE + 64 * n_in + SP_RANK * n_in + 64 * 3 + SP_NOUT + 64 * 8; }
__host__ __device__ constexpr int sp_waves(int n_in) { return n_in <= 4 ? SP_WAVES_MAX : 4; }

struct ConvArgs {
    const float* pc;
    const float* nrm;
    const float* feat_in;   // null for the first layer, else [N][n_in]
    const int32_t* nbrs;    // [N][k]
    const float* params;    // this layer's parameters, natural layout (outnet part is used from here)
    const float* wimg;      // this layer's MFMA image (SPW_FLOATS), cppf_point_encoder_pack
    float* out;             // [N][out_stride], columns 0..31 written
    int N, k, n_in, out_stride;
    float* mixed_out;       // optional [N][32 * n_in]: the contraction, kept for the backward (training)
    const int32_t* n_dev;   // *_dyn: point count in memory (N is then the capacity the launch is sized for)
    // GlobalInfoProp (models/sprin.py:75-84) in the epilogue: linear(n_out -> n_glob) per point, maximum over the workgroup's
    // points to wgmax[blockIdx][32] (plain stores: no atomics, nothing to zero); sprin_fill_kernel finishes the maximum
    const float* glob_w;    // Wa[n_glob][n_out], ba[n_glob]
    uint32_t* wgmax;
    int n_glob;
};

// hidden = {32, 64, 32, 32}, rank 32, n_out 32 (train.py:34).  Dynamic LDS: the workgroup's weight image
// (SPW_FLOATS; the bf16 kernel: SPB_WORDS), then per wave  kern[16][33] | nf[64][n_in] | contracted[32*n_in] | r[64][3] | y[32] | x6[64][8]
template <bool BF16>
__device__ __forceinline__ void sprin_conv_body(const ConvArgs& A)
{
    constexpr int IMG = BF16 ? SPB_WORDS : SPW_FLOATS;   // words of the weight image at the head of the dynamic LDS
    extern __shared__ __attribute__((aligned(16))) float sp_lds[];
    const int w = threadIdx.x >> 6, lane = lane_id();
    __shared__ uint32_t gmax[32];
    __shared__ float gw[32 * SP_NOUT + 32];   // GlobalInfoProp's weights and bias, read in the epilogue
    const int N = A.n_dev ? min(*A.n_dev, A.N) : A.N;
    if (blockIdx.x * (blockDim.x >> 6) >= N) return;   // whole workgroup past the cloud (capacity launch; a shorter member of a batch)
    if (threadIdx.x < 32) gmax[threadIdx.x] = 0u;
    for (int i = threadIdx.x; i < A.n_glob * (SP_NOUT + 1); i += blockDim.x) gw[i] = A.glob_w[i];
    const int n_in = A.n_in, k = A.k;
    const int per_wave = sp_per_wave(n_in);
    float* Wl = sp_lds;                                   // 16-byte aligned image
    float* kern = sp_lds + IMG + (size_t)w * per_wave;
    float* nf = kern + 16 * SP_KSTRIDE;
    float* contracted = nf + 64 * n_in;
    float* rr = contracted + SP_RANK * n_in;
    float* yv = rr + 64 * 3;
    float* x6l = yv + SP_NOUT;
    for (int i = threadIdx.x; i < IMG / 4; i += blockDim.x)
        reinterpret_cast<f32x4*>(Wl)[i] = reinterpret_cast<const f32x4*>(A.wimg)[i];
    const int n = blockIdx.x * (blockDim.x >> 6) + w;
    const bool live = n < N;
    const int nc = live ? n : N - 1;
    const int jc = lane < k ? lane : k - 1;
    const int nb = A.nbrs[(size_t)nc * k + jc];
    const float rx = A.pc[3 * nb], ry = A.pc[3 * nb + 1], rz = A.pc[3 * nb + 2];
    const float sx = A.pc[3 * nc], sy = A.pc[3 * nc + 1], sz = A.pc[3 * nc + 2];
    rr[3 * lane] = rx; rr[3 * lane + 1] = ry; rr[3 * lane + 2] = rz;
    __syncthreads();
    // r_mean: sequential over neighbours (every lane redundantly; LDS broadcast reads)
    float mx = 0.f, my = 0.f, mz = 0.f;
#pragma unroll 8
    for (int j = 0; j < k; ++j) { mx = mx + rr[3 * j]; my = my + rr[3 * j + 1]; mz = mz + rr[3 * j + 2]; }
    mx = mx / (float)k; my = my / (float)k; mz = mz / (float)k;
    // rifeat (models/sprin.py:40-61)
    const float l1x = mx - rx, l1y = my - ry, l1z = mz - rz;
    const float l2x = rx - sx, l2y = ry - sy, l2z = rz - sz;
    const float l3x = sx - mx, l3y = sy - my, l3z = sz - mz;
    const float l1n = norm3(l1x, l1y, l1z), l2n = norm3(l2x, l2y, l2z), l3n = norm3(l3x, l3y, l3z);
    float x6[6];
    x6[0] = l1n; x6[1] = l2n; x6[2] = l3n;
    x6[3] = ((l1x * l2x + l1y * l2y) + l1z * l2z) / (l1n * l2n + 1e-7f);
    x6[4] = ((l2x * l3x + l2y * l3y) + l2z * l3z) / (l2n * l3n + 1e-7f);
    x6[5] = ((l3x * l1x + l3y * l1y) + l3z * l1z) / (l3n * l1n + 1e-7f);
    // neighbour features
    if (A.feat_in) {
        for (int i = 0; i < n_in; ++i) nf[lane * n_in + i] = A.feat_in[(size_t)nb * n_in + i];
    } else {
        const float nax = A.nrm[3 * nb], nay = A.nrm[3 * nb + 1], naz = A.nrm[3 * nb + 2];
        const float nsx = A.nrm[3 * nc], nsy = A.nrm[3 * nc + 1], nsz = A.nrm[3 * nc + 2];
        nf[lane * 2] = l2n;                                         // |p_j - p_i|     (models/model.py:50-51)
        nf[lane * 2 + 1] = (nax * nsx + nay * nsy) + naz * nsz;     // n_j . n_i       (models/model.py:53-54)
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) x6l[lane * 8 + c] = x6[c];
    x6l[lane * 8 + 6] = 0.f; x6l[lane * 8 + 7] = 0.f;
    __syncthreads();
    // conv_kernel(6, 32, 32, 64, 32, 32) (models/sprin.py:64-72) on MFMA, 16 neighbour rows at a time -- TWO row blocks in flight
    // (sp_mfma_layer2: shared weight reads, two independent MFMA chains per output block; one block's LayerNorm under the other's
    // MFMAs), their results contracted one after the other, in neighbour order
    {
        const int j = lane & 15, g = lane >> 4;
#pragma unroll 1
        for (int rb = 0; rb < 4; rb += 2) {
            f32x4 kr[2], ks[2];
            if constexpr (BF16) {
                // the bf16 kernel-MLP (sprin_layout_bf16.h): layer 1 and the four LayerNorms as below, to the bit;
                // layers 2..5 as bf16 x bf16 products of bf(relu(LN(.))) and the packer's bf16 weights, fp32 sums on the bias seed
                f32x4 a1[2], a2[4], a3[2], a4[2];
                f32x4 b1[2], b2[4], b3[2], b4[2];
#pragma unroll
                for (int ob = 0; ob < 2; ++ob) { a1[ob] = *reinterpret_cast<const f32x4*>(Wl + SPB_B1 + 16 * ob + 4 * g); b1[ob] = a1[ob]; }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float bx = x6l[(16 * rb + j) * 8 + 4 * s + g], by = x6l[(16 * (rb + 1) + j) * 8 + 4 * s + g];
#pragma unroll
                    for (int ob = 0; ob < 2; ++ob) {
                        const float w = Wl[SPB_L1 + (ob * 2 + s) * 64 + lane];
                        a1[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, bx, a1[ob], 0, 0, 0);
                        b1[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, by, b1[ob], 0, 0, 0);
                    }
                }
                sp_ln_relu4<2>(a1, Wl + SPB_B1 + 32, Wl + SPB_B1 + 64, lane, g);
                sp_ln_relu4<2>(b1, Wl + SPB_B1 + 32, Wl + SPB_B1 + 64, lane, g);
                sp_bf16_layer2<1, 4>(Wl + SPB_L2, Wl + SPB_B2, a1, b1, a2, b2, lane, g);
                sp_ln_relu4<4>(a2, Wl + SPB_B2 + 64, Wl + SPB_B2 + 128, lane, g);
                sp_ln_relu4<4>(b2, Wl + SPB_B2 + 64, Wl + SPB_B2 + 128, lane, g);
                sp_bf16_layer2<2, 2>(Wl + SPB_L3, Wl + SPB_B3, a2, b2, a3, b3, lane, g);
                sp_ln_relu4<2>(a3, Wl + SPB_B3 + 32, Wl + SPB_B3 + 64, lane, g);
                sp_ln_relu4<2>(b3, Wl + SPB_B3 + 32, Wl + SPB_B3 + 64, lane, g);
                sp_bf16_layer2<1, 2>(Wl + SPB_L4, Wl + SPB_B4, a3, b3, a4, b4, lane, g);
                sp_ln_relu4<2>(a4, Wl + SPB_B4 + 32, Wl + SPB_B4 + 64, lane, g);
                sp_ln_relu4<2>(b4, Wl + SPB_B4 + 32, Wl + SPB_B4 + 64, lane, g);
                sp_bf16_layer2<1, 2>(Wl + SPB_L5, Wl + SPB_B5, a4, b4, kr, ks, lane, g);
            } else {
            f32x4 a1[2], a2[4], a3[2], a4[2];
            f32x4 b1[2], b2[4], b3[2], b4[2];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) { a1[ob] = *reinterpret_cast<const f32x4*>(Wl + SPW_B1 + 16 * ob + 4 * g); b1[ob] = a1[ob]; }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float bx = x6l[(16 * rb + j) * 8 + 4 * s + g], by = x6l[(16 * (rb + 1) + j) * 8 + 4 * s + g];
#pragma unroll
                for (int ob = 0; ob < 2; ++ob) {
                    const float w = Wl[SPW_L1 + (ob * 2 + s) * 64 + lane];
                    a1[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, bx, a1[ob], 0, 0, 0);
                    b1[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, by, b1[ob], 0, 0, 0);
                }
            }
            sp_ln_relu4<2>(a1, Wl + SPW_B1 + 32, Wl + SPW_B1 + 64, lane, g);
            sp_ln_relu4<2>(b1, Wl + SPW_B1 + 32, Wl + SPW_B1 + 64, lane, g);
            sp_mfma_layer2<2, 4>(Wl + SPW_L2, Wl + SPW_B2, a1, b1, a2, b2, lane, g);
            sp_ln_relu4<4>(a2, Wl + SPW_B2 + 64, Wl + SPW_B2 + 128, lane, g);
            sp_ln_relu4<4>(b2, Wl + SPW_B2 + 64, Wl + SPW_B2 + 128, lane, g);
            sp_mfma_layer2<4, 2>(Wl + SPW_L3, Wl + SPW_B3, a2, b2, a3, b3, lane, g);
            sp_ln_relu4<2>(a3, Wl + SPW_B3 + 32, Wl + SPW_B3 + 64, lane, g);
            sp_ln_relu4<2>(b3, Wl + SPW_B3 + 32, Wl + SPW_B3 + 64, lane, g);
            sp_mfma_layer2<2, 2>(Wl + SPW_L4, Wl + SPW_B4, a3, b3, a4, b4, lane, g);
            sp_ln_relu4<2>(a4, Wl + SPW_B4 + 32, Wl + SPW_B4 + 64, lane, g);
            sp_ln_relu4<2>(b4, Wl + SPW_B4 + 32, Wl + SPW_B4 + 64, lane, g);
            sp_mfma_layer2<2, 2>(Wl + SPW_L5, Wl + SPW_B5, a4, b4, kr, ks, lane, g);
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int rbh = rb + half;
#pragma unroll
                for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                    for (int r = 0; r < 4; ++r) kern[j * SP_KSTRIDE + 16 * ob + 4 * g + r] = half ? ks[ob][r] : kr[ob][r];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own LDS writes, before other lanes read them
                // einsum("bnkr,bnki->bnri") (models/sprin.py:99): contracted[r*n_in + i] accumulates these 16 neighbours,
                // sequentially and in neighbour order across the row blocks
                const int jn = min(16, k - 16 * rbh);
                for (int t = lane; t < SP_RANK * n_in; t += 64) {
                    const int r = t / n_in, i = t - r * n_in;
                    float acc = rbh == 0 ? 0.f : contracted[t];
#pragma unroll 8
                    for (int jj = 0; jj < jn; ++jj) acc = fmaf(kern[jj * SP_KSTRIDE + r], nf[(16 * rbh + jj) * n_in + i], acc);
                    contracted[t] = acc;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (kern is rewritten by the other half / the next trip)
            }
        }
    }
    const float* p = A.params + SP_NAT_KERNEL;   // outnet parameters follow the kernel-MLP in the natural layout
    const int C = SP_RANK * n_in;
    if (A.mixed_out && live)
        for (int t = lane; t < C; t += 64) A.mixed_out[(size_t)n * C + t] = contracted[t];
    __syncthreads();
    // outnet (transposed weights: lane o reads Wo_t[c][o], coalesced) + LayerNorm (models/sprin.py:100,105)
    const float* Wo = p;
    const float* bo = Wo + (size_t)C * SP_NOUT;
    const int o = lane & (SP_NOUT - 1);
    float acc = bo[o];
#pragma unroll 8
    for (int c = 0; c < C; ++c) acc = fmaf(Wo[(size_t)c * SP_NOUT + o], contracted[c], acc);
    if (lane < SP_NOUT) yv[lane] = acc;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < SP_NOUT; ++q) s = s + yv[q];
    const float mean = s / (float)SP_NOUT;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < SP_NOUT; ++q) { const float dd = yv[q] - mean; v = v + dd * dd; }
    const float inv = inv_sqrt_rn(v / (float)SP_NOUT + 1e-5f);   // = 1.0f / sqrtf(.), bit for bit
    const float z = ((acc - mean) * inv) * bo[SP_NOUT + o] + bo[2 * SP_NOUT + o];
    if (live && lane < SP_NOUT) A.out[(size_t)n * A.out_stride + lane] = z;
    // GlobalInfoProp's linear on the row just written: lane g owns channel g, a bias-seeded fmaf chain over ascending input
    // index (what sprin_glob_kernel did with one thread per point and 32 strided reads of the row), then the maximum -- exact
    // in any order -- over the workgroup's points
    if (lane < SP_NOUT) yv[lane] = z;     // (this wave's reads of yv above are done: LDS operations of a wave stay in order)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int gch = lane < A.n_glob ? lane : 0;
    const float* Wa = gw + gch * SP_NOUT;
    float ga = gw[A.n_glob * SP_NOUT + gch];
#pragma unroll 8
    for (int q = 0; q < SP_NOUT; ++q) ga = fmaf(Wa[q], yv[q], ga);
    if (live && lane < A.n_glob) atomicMax(&gmax[lane], f2ord(ga));
    __syncthreads();
    if (threadIdx.x < 32) A.wgmax[(size_t)blockIdx.x * 32 + threadIdx.x] = gmax[threadIdx.x];
}

// ... and the members' convolutions in one launch (blockIdx.y = member: its own cloud, neighbour sets, weight image -- members of
// different categories carry different encoders -- and output)
struct ConvBatch { ConvArgs item[SP_BATCH_MAX]; };

// ---- host side
inline int64_t conv_params(const int32_t* hidden, int n_hidden, int rank, int n_in, int n_out)
{
    int64_t n = 0;
    int in = 6;
    for (int i = 0; i < n_hidden; ++i) { n += (int64_t)hidden[i] * in + 3 * hidden[i]; in = hidden[i]; }
    n += (int64_t)rank * in + rank;
    n += (int64_t)rank * n_in * n_out + 3 * n_out;
    return n;
}
inline bool sp_std_shape(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob)
{
    return n_hidden == 4 && hidden[0] == 32 && hidden[1] == 64 && hidden[2] == 32 && hidden[3] == 32 && rank == SP_RANK &&
           n_out == SP_NOUT && n_glob >= 1 && n_glob <= 32 && n_nbr_feats == 2;
}
inline size_t sp_natural_floats(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                int num_layers)
{
    size_t n = 0;
    for (int l = 0; l < num_layers; ++l)
        n += (size_t)conv_params(hidden, n_hidden, rank, l == 0 ? n_nbr_feats : n_out + n_glob, n_out) +
             (size_t)n_glob * n_out + n_glob;
    return n;
}

// What a precision brings to the shared host code: the words of one layer's weight image (it leads the dynamic LDS) and the
// launches of its two kernels (each sets the kernel's dynamic-LDS limit first and returns a HIP status).
struct SpVariant {
    int image_words;
    int (*conv)(const ConvArgs& A, unsigned blocks, int waves, size_t lds_bytes, hipStream_t st);
    int (*conv_batch)(const ConvBatch& B, dim3 grid, int waves, size_t lds_bytes, hipStream_t st);
};

}  // namespace sprin

// (sprin.hip) cppf_point_encoder_forward / _forward_dyn / _forward_train and cppf_point_encoder_forward_batch for either precision:
// `packed` = the natural block followed by one image of V.image_words per layer
int cppf_internal_sprin_forward(const sprin::SpVariant& V, const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k,
                                const float* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                int n_glob, int num_layers, float* out, float* mixed_out, void* workspace, size_t workspace_bytes,
                                void* stream, const int32_t* n_dev);
int cppf_internal_sprin_forward_batch(const sprin::SpVariant& V, int n_items, const CppfPointEncItem* items, int k,
                                      const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                      int num_layers, void* stream);
