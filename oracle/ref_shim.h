/*
 * ref_shim.h -- what the reference's helper_math.cuh expects from the CUDA runtime header, supplied by us so that the
 * reference's own vote-kernel text (models/voting.py, extracted at build time into oracle/_ref/ by ref_build.py) compiles
 * (a) as host C++ with g++ and (b) as a gfx950 code object with hipcc.  TEST INFRASTRUCTURE ONLY; all of this text is ours.
 *
 * The copy of helper_math.cuh under oracle/_ref/ has its one CUDA-toolkit include line redirected to this file.
 *
 * Host build: plain structs for the vector types, the base make_* constructors, min / max, rsqrtf, the launch indices
 * as globals that the entry points (ref_host_entry.cpp) step serially, and a serial atomicAdd.  __CUDACC__ is defined so
 * that helper_math.cuh leaves fminf / fmaxf / min / max to us and to <math.h>.  cos / sin / tan of a float resolve to
 * the float overloads of <math.h> (glibc cosf / sinf / tanf), as they resolve to the float functions under CUDA.
 *
 * Device build: <hip/hip_runtime.h> brings blockIdx, atomicAdd, min / max and the device libm (ocml).  Its own vector
 * types carry operators that collide with helper_math.cuh's, so the type names and make_* are renamed to plain structs
 * of ours before the reference text is read.
 */
#ifndef CPPF_REF_SHIM_H
#define CPPF_REF_SHIM_H

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define REF_HD __host__ __device__
#define float2 ref_float2
#define float3 ref_float3
#define float4 ref_float4
#define int2 ref_int2
#define int3 ref_int3
#define int4 ref_int4
#define uint2 ref_uint2
#define uint3 ref_uint3
#define uint4 ref_uint4
#define make_float2 ref_make_float2
#define make_float3 ref_make_float3
#define make_float4 ref_make_float4
#define make_int2 ref_make_int2
#define make_int3 ref_make_int3
#define make_int4 ref_make_int4
#define make_uint2 ref_make_uint2
#define make_uint3 ref_make_uint3
#define make_uint4 ref_make_uint4
#else
#include <math.h>
#define REF_HD
#define __host__
#define __device__
#define __global__
struct ref_launch_index { unsigned int x, y, z; };
static ref_launch_index blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, threadIdx = {0, 0, 0};
static inline int max(int a, int b) { return a > b ? a : b; }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
static inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float atomicAdd(float* p, float v) { float o = *p; *p = o + v; return o; }   /* one thread at a time */
#endif

#ifndef __CUDACC__
#define __CUDACC__ 1
#endif
#ifdef M_PI            /* the kernel text defines its own */
#undef M_PI
#endif

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct uint3 { unsigned int x, y, z; };
struct uint4 { unsigned int x, y, z, w; };

static inline REF_HD float2 make_float2(float x, float y) { float2 r = {x, y}; return r; }
static inline REF_HD float3 make_float3(float x, float y, float z) { float3 r = {x, y, z}; return r; }
static inline REF_HD float4 make_float4(float x, float y, float z, float w) { float4 r = {x, y, z, w}; return r; }
static inline REF_HD int2 make_int2(int x, int y) { int2 r = {x, y}; return r; }
static inline REF_HD int3 make_int3(int x, int y, int z) { int3 r = {x, y, z}; return r; }
static inline REF_HD int4 make_int4(int x, int y, int z, int w) { int4 r = {x, y, z, w}; return r; }
static inline REF_HD uint2 make_uint2(unsigned int x, unsigned int y) { uint2 r = {x, y}; return r; }
static inline REF_HD uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { uint3 r = {x, y, z}; return r; }
static inline REF_HD uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w)
{
    uint4 r = {x, y, z, w};
    return r;
}

#endif
