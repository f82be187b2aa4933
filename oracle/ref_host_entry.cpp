/*
 * ref_host_entry.cpp -- C entry points over the reference's own vote-kernel text, compiled as host C++.
 *
 * TEST INFRASTRUCTURE ONLY.  The three files included below are not in this repository: oracle/ref_build.py extracts them
 * at build time from the reference's models/voting.py into oracle/_ref/ (git-ignored) together with a copy of
 * helper_math.cuh whose CUDA-toolkit include is redirected to oracle/ref_shim.h.  Built with contraction off and glibc's
 * cosf / sinf / tanf, so that what this library computes is the reference's text under the arithmetic of
 * oracle/voting_variants.c's ORV_LIBM member, bit for bit (tests/test_ref_vote_cpu.py).
 *
 * Each entry point zero-fills the kernel's output, then steps the launch indices serially over the reference's launch
 * convention: blocks of 32 threads, ceil(n_ppfs / 32) blocks (nocs/inference.py:192-275 launches at least that many).
 * Compiled a second time with -x hip --genco (REF_DEVICE_ONLY) the same file yields the gfx950 code object, kernels only.
 */
#include "ppf_voting.cu.inc"
#include "backvote.cu.inc"
#include "rot_voting.cu.inc"

#ifndef REF_DEVICE_ONLY
#include <stdint.h>
#include <string.h>

#define REF_FOR_EACH_THREAD(n)                                                        \
    blockDim.x = 32;                                                                  \
    for (blockIdx.x = 0; (int64_t)blockIdx.x * 32 < (int64_t)(n); ++blockIdx.x)       \
        for (threadIdx.x = 0; threadIdx.x < 32; ++threadIdx.x)

extern "C" void ref_host_ppf_voting(const float* points, const float* outputs, const float* probs, const int* point_idxs,
                                    float* grid_obj, const float* corner, float res, int n_ppfs, int n_rots, int gx, int gy,
                                    int gz, int adaptive)
{
    memset(grid_obj, 0, sizeof(float) * (size_t)gx * gy * gz);
    REF_FOR_EACH_THREAD(n_ppfs)
    ppf_voting(points, outputs, probs, point_idxs, grid_obj, corner, res, n_ppfs, n_rots, gx, gy, gz, adaptive != 0);
}

extern "C" void ref_host_backvote(const float* points, const float* outputs, float* out_offsets, const int* point_idxs,
                                  const float* corner, float res, int n_ppfs, int n_rots, int gx, int gy, int gz,
                                  const float* gt_center, float tol)
{
    memset(out_offsets, 0, sizeof(float) * 3 * (size_t)n_ppfs);
    REF_FOR_EACH_THREAD(n_ppfs)
    backvote(points, outputs, (float3*)out_offsets, point_idxs, corner, res, n_ppfs, n_rots, gx, gy, gz, gt_center, tol);
}

extern "C" void ref_host_rot_voting(const float* points, const float* preds_rot, float* outputs_up, const int* point_idxs,
                                    const float* corner, float res, int n_ppfs, int n_rots, int gx, int gy, int gz)
{
    memset(outputs_up, 0, sizeof(float) * 3 * (size_t)n_ppfs * n_rots);
    REF_FOR_EACH_THREAD(n_ppfs)
    rot_voting(points, (const float*)0, preds_rot, (float3*)outputs_up, point_idxs, corner, res, n_ppfs, n_rots, gx, gy, gz);
}
#endif
