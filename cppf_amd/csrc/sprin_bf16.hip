// bf16 point encoder for gfx950: the SPRIN convolution of sprin.hip with the hidden layers of its kernel-MLP on
// v_mfma_f32_16x16x32_bf16.  Opt-in (PointEncoder.set_precision("bf16")); the fp32 kernels stay the default and are not touched by
// this file.
//
// Numerics (tests/sprin_bf16_ref.py is the CPU statement).  bf() = round to nearest even to bf16.
//   gather, rifeat          fp32, the fp32 kernel's own code
//   layer 1 (6 -> 32)       fp32, the fp32 kernel's own v_mfma_f32_16x16x4_f32 steps on the fp32 section of the image
//   LayerNorm 1..4 + ReLU   fp32 on the fp32 accumulators (sp_ln_relu4)
//   layers 2..4             y = bf(W) . bf(relu(LN(y_prev))) + b      bf16 x bf16 products, fp32 sums on the bias seed
//   layer 5                 kern = bf(W5) . bf(relu(LN4(y4))) + b5    fp32, not rounded
//   contraction, outnet, LayerNorm, GlobalInfoProp, fill: the fp32 code, reading the fp32 kern.
// Per 16-neighbour row block: 4 fp32 MFMAs + 4 + 4 + 2 + 2 of the K = 32 bf16 form, against 100 fp32 ones.
//
// Everything but the kernel-MLP is sprin_conv.h's shared body (template parameter BF16) and sprin.hip's shared host code
// (cppf_internal_sprin_forward / _batch: the search, the fill kernels, the workspace contract, the `n_dev` and batch handling).
#include <string.h>
#include "sprin_conv.h"

using namespace sprin;

namespace {

__global__ __launch_bounds__(SP_WAVES_MAX * 64) void sprin_conv_bf16_kernel(ConvArgs A) { sprin_conv_body<true>(A); }
__global__ __launch_bounds__(SP_WAVES_MAX * 64) void sprin_conv_bf16_batch_kernel(ConvBatch B) { sprin_conv_body<true>(B.item[blockIdx.y]); }

int launch_conv(const ConvArgs& A, unsigned blocks, int waves, size_t lds, hipStream_t st)
{
    hipError_t e = hipFuncSetAttribute((const void*)sprin_conv_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    sprin_conv_bf16_kernel<<<blocks, waves * 64, lds, st>>>(A);
    return 0;
}
int launch_conv_batch(const ConvBatch& B, dim3 grid, int waves, size_t lds, hipStream_t st)
{
    hipError_t e = hipFuncSetAttribute((const void*)sprin_conv_bf16_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    sprin_conv_bf16_batch_kernel<<<grid, waves * 64, lds, st>>>(B);
    return 0;
}
const SpVariant SP_BF16 = {SPB_WORDS, launch_conv, launch_conv_batch};

// natural floats of layer l, and where it starts
struct LayerSpan { size_t begin, floats; };
LayerSpan layer_span(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob, int l)
{
    return {sp_natural_floats(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, l),
            (size_t)conv_params(hidden, n_hidden, rank, l == 0 ? n_nbr_feats : n_out + n_glob, n_out) + (size_t)n_glob * n_out + n_glob};
}

__global__ __launch_bounds__(256) void sprin_pack_bf16_kernel(const float* __restrict__ natural_layer, uint32_t* __restrict__ image)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < SPB_WORDS) image[i] = sp_bf16_image_word(i, natural_layer);
}

}  // namespace

extern "C" {

size_t cppf_point_encoder_bf16_packed_bytes(const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                            int num_layers)
{
    if (!hidden || n_hidden <= 0 || num_layers <= 0) return 0;
    if (!sp_std_shape(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob)) return 0;
    return (sp_natural_floats(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, num_layers) + (size_t)num_layers * SPB_WORDS) * 4;
}

// natural parameters (host) -> image (host buffer): the natural block verbatim (the outnet and GlobalInfoProp read it), then one
// SPB_WORDS image of the kernel-MLP per layer
int cppf_point_encoder_bf16_pack(const float* natural, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                 int n_glob, int num_layers, void* out)
{
    if (!natural || !hidden || !out || n_hidden <= 0 || num_layers <= 0) return CPPF_EINVAL;
    if (!sp_std_shape(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob)) return CPPF_EUNSUPPORTED;
    const size_t nat = sp_natural_floats(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, num_layers);
    memcpy(out, natural, nat * sizeof(float));
    uint32_t* images = static_cast<uint32_t*>(out) + nat;
    for (int l = 0; l < num_layers; ++l) {
        const LayerSpan sp = layer_span(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, l);
        for (int i = 0; i < SPB_WORDS; ++i) images[(size_t)l * SPB_WORDS + i] = sp_bf16_image_word(i, natural + sp.begin);
    }
    return 0;
}

int cppf_point_encoder_bf16_pack_device(const float* natural, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                        int n_glob, int num_layers, void* packed, void* stream)
{
    if (!natural || !hidden || !packed || n_hidden <= 0 || num_layers <= 0) return CPPF_EINVAL;
    if (!sp_std_shape(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob)) return CPPF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t nat = sp_natural_floats(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, num_layers);
    hipError_t e = hipMemcpyAsync(packed, natural, nat * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    uint32_t* images = static_cast<uint32_t*>(packed) + nat;
    for (int l = 0; l < num_layers; ++l) {
        const LayerSpan sp = layer_span(hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, l);
        sprin_pack_bf16_kernel<<<(SPB_WORDS + 255) / 256, 256, 0, st>>>(natural + sp.begin, images + (size_t)l * SPB_WORDS);
    }
    return (int)hipGetLastError();
}

int cppf_point_encoder_bf16_forward(const float* pc, const float* nrm, const int32_t* nbrs, int n_points, int k, const void* packed,
                                    const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out, int n_glob,
                                    int num_layers, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    return cppf_internal_sprin_forward(SP_BF16, pc, nrm, nbrs, n_points, k, static_cast<const float*>(packed), hidden, n_hidden, rank,
                                       n_nbr_feats, n_out, n_glob, num_layers, out, nullptr, workspace, workspace_bytes, stream, nullptr);
}

int cppf_point_encoder_bf16_forward_dyn(const float* pc, const float* nrm, const int32_t* nbrs, int n_cap, const int32_t* n_dev, int k,
                                        const void* packed, const int32_t* hidden, int n_hidden, int rank, int n_nbr_feats, int n_out,
                                        int n_glob, int num_layers, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!n_dev) return CPPF_EINVAL;
    return cppf_internal_sprin_forward(SP_BF16, pc, nrm, nbrs, n_cap, k, static_cast<const float*>(packed), hidden, n_hidden, rank,
                                       n_nbr_feats, n_out, n_glob, num_layers, out, nullptr, workspace, workspace_bytes, stream, n_dev);
}

// CppfPointEncItem.packed points at each member's bf16 image
int cppf_point_encoder_bf16_forward_batch(int n_items, const CppfPointEncItem* items, int k, const int32_t* hidden, int n_hidden,
                                          int rank, int n_nbr_feats, int n_out, int n_glob, int num_layers, void* stream)
{
    return cppf_internal_sprin_forward_batch(SP_BF16, n_items, items, k, hidden, n_hidden, rank, n_nbr_feats, n_out, n_glob, num_layers,
                                             stream);
}

}  // extern "C"
