/*
 * ref_runner.c -- runs one kernel of a vote code object (oracle/_ref/ref_vote_gfx950*.hsaco, the reference's own kernel
 * text compiled for gfx950 by oracle/ref_build.py) on HIP device 0.  Plain C over libamdhip64.
 *
 * TEST INFRASTRUCTURE ONLY: started by tests/test_gpu_ref_vote.py as a fresh child process.
 *
 *   ref_vote_runner <code object> <ppf_voting|backvote|rot_voting> <input file> <output file>
 *
 * Input file (little endian, written by tests/ref_vote_cases.py:write_job):
 *   int32[8]  n_points, n_ppfs, n_rots, gx, gy, gz, adaptive, 0
 *   float[2]  res, tol
 *   float     points[n_points*3], outputs[n_ppfs*2], probs[n_points]
 *   int32     point_idxs[n_ppfs*2]
 *   float     corner[3], gt_center[3], preds_rot[n_ppfs]
 * Output file: the kernel's output array, zero-filled before the launch:
 *   ppf_voting float[gx*gy*gz], backvote float[n_ppfs*3], rot_voting float[n_ppfs*n_rots*3].
 * Launch: blocks of 32 threads, ceil(n_ppfs / 32) blocks, the reference's own convention.
 * Checked on the host first: the header's ranges, that the file is exactly as long as its header says, and every point
 * index.  A one-shot process: on any error it reports and exits at once, and leaves its memory, its file and the HIP
 * context to the exit.  Exit status: 0 ok, 2 usage / bad input, 3 HIP error.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CK(call)                                                                                      \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ref_vote_runner: %s -> %s\n", #call, hipGetErrorString(e_));             \
            return 3;                                                                                 \
        }                                                                                             \
    } while (0)

static int bad(const char* what)
{
    fprintf(stderr, "ref_vote_runner: %s\n", what);
    return 2;
}

static void* rd(FILE* f, size_t n_bytes)
{
    void* p = malloc(n_bytes ? n_bytes : 1);
    if (!p || fread(p, 1, n_bytes, f) != n_bytes) { free(p); return NULL; }
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 5) return bad("usage: ref_vote_runner <code object> <kernel> <input> <output>");
    const char* kname = argv[2];
    const int which = !strcmp(kname, "ppf_voting") ? 0 : !strcmp(kname, "backvote") ? 1 : !strcmp(kname, "rot_voting") ? 2 : -1;
    if (which < 0) return bad("unknown kernel");
    FILE* f = fopen(argv[3], "rb");
    if (!f) return bad("cannot open the input file");
    int32_t h[8];
    float rt[2];
    if (fread(h, 4, 8, f) != 8 || fread(rt, 4, 2, f) != 2) { fclose(f); return bad("short header"); }
    const int n_points = h[0], n_ppfs = h[1], n_rots = h[2], gx = h[3], gy = h[4], gz = h[5];
    unsigned char adaptive = h[6] != 0;
    float res = rt[0], tol = rt[1];
    if (n_points < 1 || n_points > (1 << 24) || n_ppfs < 1 || n_ppfs > (1 << 24) || n_rots < 1 || n_rots > 360 || gx < 2 ||
        gy < 2 || gz < 2 || gx > 2048 || gy > 2048 || gz > 2048 || (int64_t)gx * gy * gz > ((int64_t)1 << 28) || !(res > 0.f))
    {
        fclose(f);
        return bad("header out of range");
    }
    const size_t np3 = (size_t)n_points * 3, pp2 = (size_t)n_ppfs * 2;
    float* points = (float*)rd(f, np3 * 4);
    float* outputs = (float*)rd(f, pp2 * 4);
    float* probs = (float*)rd(f, (size_t)n_points * 4);
    int32_t* idxs = (int32_t*)rd(f, pp2 * 4);
    float* corner = (float*)rd(f, 12);
    float* gt = (float*)rd(f, 12);
    float* rot = (float*)rd(f, (size_t)n_ppfs * 4);
    const int trailing = fgetc(f) != EOF;
    fclose(f);
    if (!points || !outputs || !probs || !idxs || !corner || !gt || !rot) return bad("short input file");
    if (trailing) return bad("input file longer than its header says");
    for (size_t i = 0; i < pp2; ++i)
        if (idxs[i] < 0 || idxs[i] >= n_points) return bad("point index out of range");
    /* ppf_voting writes cells floor+{0,1} of coordinates it has tested to lie in [0.01, dim-1.01): in bounds for any input */
    const size_t n_out = which == 0 ? (size_t)gx * gy * gz : which == 1 ? (size_t)n_ppfs * 3 : (size_t)n_ppfs * n_rots * 3;

    hipModule_t mod;
    hipFunction_t fn;
    CK(hipSetDevice(0));
    CK(hipModuleLoad(&mod, argv[1]));
    CK(hipModuleGetFunction(&fn, mod, kname));
    void *d_points, *d_outputs, *d_probs, *d_idxs, *d_corner, *d_gt, *d_rot, *d_out;
    CK(hipMalloc(&d_points, np3 * 4));
    CK(hipMalloc(&d_outputs, pp2 * 4));
    CK(hipMalloc(&d_probs, (size_t)n_points * 4));
    CK(hipMalloc(&d_idxs, pp2 * 4));
    CK(hipMalloc(&d_corner, 12));
    CK(hipMalloc(&d_gt, 12));
    CK(hipMalloc(&d_rot, (size_t)n_ppfs * 4));
    CK(hipMalloc(&d_out, n_out * 4));
    CK(hipMemcpy(d_points, points, np3 * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_outputs, outputs, pp2 * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_probs, probs, (size_t)n_points * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_idxs, idxs, pp2 * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_corner, corner, 12, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_gt, gt, 12, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_rot, rot, (size_t)n_ppfs * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0, n_out * 4));

    int n = n_ppfs, nr = n_rots, x = gx, y = gy, z = gz;
    void* a_ppf[] = {&d_points, &d_outputs, &d_probs, &d_idxs, &d_out, &d_corner, &res, &n, &nr, &x, &y, &z, &adaptive};
    void* a_back[] = {&d_points, &d_outputs, &d_out, &d_idxs, &d_corner, &res, &n, &nr, &x, &y, &z, &d_gt, &tol};
    void* a_rot[] = {&d_points, &d_outputs, &d_rot, &d_out, &d_idxs, &d_corner, &res, &n, &nr, &x, &y, &z};
    void** args = which == 0 ? a_ppf : which == 1 ? a_back : a_rot;
    CK(hipModuleLaunchKernel(fn, (unsigned)((n_ppfs + 31) / 32), 1, 1, 32, 1, 1, 0, NULL, args, NULL));
    CK(hipDeviceSynchronize());

    float* out = (float*)malloc(n_out * 4);
    if (!out) return bad("out of memory");
    CK(hipMemcpy(out, d_out, n_out * 4, hipMemcpyDeviceToHost));
    CK(hipModuleUnload(mod));
    FILE* g = fopen(argv[4], "wb");
    if (!g) return bad("cannot write the output file");
    const int wrote = fwrite(out, 4, n_out, g) == n_out;
    if (fclose(g) != 0 || !wrote) return bad("cannot write the output file");
    return 0;
}
