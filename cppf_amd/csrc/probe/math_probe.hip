// Test-only probes of the shared device arithmetic (csrc/cppf_math.h, vote_common.h, backvote_common.h): every entry maps ONE
// primitive of those headers over device arrays, one lane per element, so that tests/test_gpu_device_math.py can hold each
// primitive to the contract its comment states.  The headers are included, never copied: a change to them changes what is
// tested.  Built into libcppf_probe.so (csrc/Makefile), never into libcppf_hip.so, twice: with the library's default flags
// (symbols probe_*) and with the additional flags of pair_mlp.o (-DPROBE_PREFIX=probe_nonans_: symbols probe_nonans_*).
//
// The sweep_* entries walk a range of bit patterns on the device and compare the primitive with the compiler's own IEEE
// operation (`a / b` through a volatile, sqrtf, 1.0f / sqrtf): out[0] = number of mismatches (one ballot-counted integer add
// per wave), out[1] = the smallest mismatching operand bits (all ones: none).
// Plain C++ only: ordinary vector stores, integer atomics, no inline assembly.  Every entry returns a hipError_t as int.
#include "../cppf_math.h"
#include "../vote_common.h"
#include "../backvote_common.h"

#ifndef PROBE_PREFIX
#define PROBE_PREFIX probe_
#endif
#define PROBE_CAT2(a, b) a##b
#define PROBE_CAT(a, b) PROBE_CAT2(a, b)
#define PN(name) PROBE_CAT(PROBE_PREFIX, name)

#define PROBE_THREADS 256
#define PROBE_SWEEP_BLOCKS 4096

namespace PN(kernels) {

static inline int map_blocks(int64_t n) { return (int)((n + PROBE_THREADS - 1) / PROBE_THREADS < 65536 ? (n + PROBE_THREADS - 1) / PROBE_THREADS : 65536); }

#define PROBE_MAP_LOOP(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x; i < (n); i += (int64_t)gridDim.x * PROBE_THREADS)

__global__ void __launch_bounds__(PROBE_THREADS) k_div_by(const float* a, const float* b, float* q, int64_t n)
{
    PROBE_MAP_LOOP(i, n) q[i] = div_by(a[i], b[i], refined_rcp(b[i]));
}
__global__ void __launch_bounds__(PROBE_THREADS) k_sqrt_rn(const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = sqrt_rn(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_inv_sqrt_rn(const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = inv_sqrt_rn(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_sub3(const float* a, const float* b, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) {
        const f3 d = sub3(ld3(a, (int)i), ld3(b, (int)i));
        r[3 * i] = d.x; r[3 * i + 1] = d.y; r[3 * i + 2] = d.z;
    }
}
__global__ void __launch_bounds__(PROBE_THREADS) k_exp2w(const float* l, const float* c, float* w, int64_t n)
{
    PROBE_MAP_LOOP(i, n) w[i] = det_exp2w(l[i], c[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_sincos(const double* x, double* s, double* c, int64_t n)
{
    PROBE_MAP_LOOP(i, n) { double ss, cc; det_sincos(x[i], &ss, &cc); s[i] = ss; c[i] = cc; }
}
__global__ void __launch_bounds__(PROBE_THREADS) k_rot_cs(const int* ri, const int* rn, float* cs, float* sn, int64_t n)
{
    PROBE_MAP_LOOP(i, n) { const float2 v = rot_cs(ri[i], rn[i]); cs[i] = v.x; sn[i] = v.y; }
}
__global__ void __launch_bounds__(PROBE_THREADS) k_tanf(const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = det_tanf(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_atan01(const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = atan01_approx(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_atan2(const float* y, const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = atan2_approx(y[i], x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_acos(const float* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = acos_approx(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_f2ord(const float* x, uint32_t* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = f2ord(x[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_ord2f(const uint32_t* x, float* r, int64_t n)
{
    PROBE_MAP_LOOP(i, n) r[i] = ord2f(x[i]);
}
// whole workgroups only (n a multiple of 256, one element per lane): the wave helpers expect 64 active lanes
__global__ void __launch_bounds__(PROBE_THREADS) k_wave_incl_scan(const int* v, int* r)
{
    const int64_t i = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    r[i] = wave_incl_scan(v[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_wave_max_u64(const unsigned long long* v, unsigned long long* r)
{
    const int64_t i = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    r[i] = wave_max_u64(v[i]);
}
__global__ void __launch_bounds__(PROBE_THREADS) k_bv_arc(const float* L2, const float* w, const float* x, const float* y, const float* tol,
                                                          const int* nr, const float* cmax, int* lo, int* cnt, int64_t n)
{
    PROBE_MAP_LOOP(i, n) {
        const int2 a = bv_arc(L2[i], ld3(w, (int)i), ld3(x, (int)i), ld3(y, (int)i), tol[i], nr[i], cmax[i]);
        lo[i] = a.x; cnt[i] = a.y;
    }
}

// ----------------------------------------------------------------------------- sweeps
__device__ __forceinline__ void sweep_note(bool bad, unsigned long long operand, unsigned long long* out)
{
    const unsigned long long m = __ballot(bad);
    if (m == 0) return;
    if (bad) atomicMin(out + 1, operand);
    if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(out, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// sqrt_rn against sqrtf over the bit patterns [first, first + count)
__global__ void __launch_bounds__(PROBE_THREADS) k_sweep_sqrt(uint32_t first, uint64_t count, unsigned long long* out)
{
    const uint64_t trips = (count + (uint64_t)gridDim.x * PROBE_THREADS - 1) / ((uint64_t)gridDim.x * PROBE_THREADS);
    for (uint64_t t = 0; t < trips; ++t) {                         // (wave-uniform trip count: the ballot sees whole waves)
        const uint64_t i = (t * gridDim.x + blockIdx.x) * PROBE_THREADS + threadIdx.x;
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        sweep_note(i < count && !same_bits(sqrt_rn(x), sqrtf(x)), bits, out);
    }
}
// inv_sqrt_rn against 1.0f / sqrtf over the bit patterns [first, first + count)
__global__ void __launch_bounds__(PROBE_THREADS) k_sweep_inv_sqrt(uint32_t first, uint64_t count, unsigned long long* out)
{
    const uint64_t trips = (count + (uint64_t)gridDim.x * PROBE_THREADS - 1) / ((uint64_t)gridDim.x * PROBE_THREADS);
    for (uint64_t t = 0; t < trips; ++t) {
        const uint64_t i = (t * gridDim.x + blockIdx.x) * PROBE_THREADS + threadIdx.x;
        const uint32_t bits = first + (uint32_t)i;
        const float x = __uint_as_float(bits);
        volatile float s = sqrtf(x);
        sweep_note(i < count && !same_bits(inv_sqrt_rn(x), 1.0f / s), bits, out);
    }
}
// div_by(+-a, b) against +-a / b for one denominator b and the numerator magnitudes with bits [first, first + count)
__global__ void __launch_bounds__(PROBE_THREADS) k_sweep_div(float b, uint32_t first, uint64_t count, unsigned long long* out)
{
    const float y = refined_rcp(b);
    volatile float bb = b;
    const uint64_t trips = (count + (uint64_t)gridDim.x * PROBE_THREADS - 1) / ((uint64_t)gridDim.x * PROBE_THREADS);
    for (uint64_t t = 0; t < trips; ++t) {
        const uint64_t i = (t * gridDim.x + blockIdx.x) * PROBE_THREADS + threadIdx.x;
        const uint32_t bits = first + (uint32_t)i;
        const float a = __uint_as_float(bits);
        const bool bad = !same_bits(div_by(a, b, y), a / bb) || !same_bits(div_by(-a, b, y), -a / bb);
        sweep_note(i < count && bad, bits, out);
    }
}
// The PPF's divisions (pair_mlp_common.h:ppf_from): a / (d + 1e-7f) for the distances d with bits [first, first + count) and the
// numerators a = fl(d r) and fl(-d r), r = 1 - k / n_ratio, k = 0 .. n_ratio - 1: |a| <= d, as the components of a difference vector
// are against its length.  operand = d's bits << 32 | k.
__global__ void __launch_bounds__(PROBE_THREADS) k_sweep_div_ppf(uint32_t first, uint64_t count, int n_ratio, unsigned long long* out)
{
    const float step = 1.0f / (float)n_ratio;                      // n_ratio a power of two: k * step is exact
    const uint64_t trips = (count + (uint64_t)gridDim.x * PROBE_THREADS - 1) / ((uint64_t)gridDim.x * PROBE_THREADS);
    for (uint64_t t = 0; t < trips; ++t) {
        const uint64_t i = (t * gridDim.x + blockIdx.x) * PROBE_THREADS + threadIdx.x;
        const uint32_t bits = first + (uint32_t)i;
        const float d = __uint_as_float(bits);
        const float den = d + 1e-7f, y = refined_rcp(den);
        volatile float dd = den;
        int bad_k = -1;
        for (int k = n_ratio - 1; k >= 0; --k) {
            const float a = d * (1.0f - (float)k * step);
            // (d = 0: the numerator -0 is div_by's stated exception, cppf_math.h; +0 is compared)
            const bool bad = !same_bits(div_by(a, den, y), a / dd) || (a != 0.f && !same_bits(div_by(-a, den, y), -a / dd));
            bad_k = bad ? k : bad_k;
        }
        sweep_note(i < count && bad_k >= 0, (unsigned long long)bits << 32 | (unsigned)max(bad_k, 0), out);
    }
}

static int sweep_begin(unsigned long long* out, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    return (int)hipMemsetAsync(out + 1, 0xff, sizeof(unsigned long long), st);
}

}  // namespace PN(kernels)

using namespace PN(kernels);

#define PROBE_MAP(kernel, n, stream, ...)                                                                   \
    do {                                                                                                    \
        if ((n) < 0) return (int)hipErrorInvalidValue;                                                      \
        if ((n) == 0) return 0;                                                                             \
        hipLaunchKernelGGL(kernel, dim3(map_blocks(n)), dim3(PROBE_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__); \
        CPPF_CHECK_LAUNCH();                                                                                \
        return 0;                                                                                           \
    } while (0)

extern "C" {

int PN(div_by)(const float* a, const float* b, float* q, int64_t n, void* stream) { PROBE_MAP(k_div_by, n, stream, a, b, q, n); }
int PN(sqrt_rn)(const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_sqrt_rn, n, stream, x, r, n); }
int PN(inv_sqrt_rn)(const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_inv_sqrt_rn, n, stream, x, r, n); }
/* a, b, r: f32[n,3], n < 2^29 */
int PN(sub3)(const float* a, const float* b, float* r, int64_t n, void* stream)
{
    if (n >= ((int64_t)1 << 29)) return (int)hipErrorInvalidValue;
    PROBE_MAP(k_sub3, n, stream, a, b, r, n);
}
int PN(det_exp2w)(const float* l, const float* c, float* w, int64_t n, void* stream) { PROBE_MAP(k_exp2w, n, stream, l, c, w, n); }
int PN(det_sincos)(const double* x, double* s, double* c, int64_t n, void* stream) { PROBE_MAP(k_sincos, n, stream, x, s, c, n); }
int PN(rot_cs)(const int* i, const int* nr, float* cs, float* sn, int64_t n, void* stream) { PROBE_MAP(k_rot_cs, n, stream, i, nr, cs, sn, n); }
int PN(det_tanf)(const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_tanf, n, stream, x, r, n); }
int PN(atan01_approx)(const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_atan01, n, stream, x, r, n); }
int PN(atan2_approx)(const float* y, const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_atan2, n, stream, y, x, r, n); }
int PN(acos_approx)(const float* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_acos, n, stream, x, r, n); }
int PN(f2ord)(const float* x, uint32_t* r, int64_t n, void* stream) { PROBE_MAP(k_f2ord, n, stream, x, r, n); }
int PN(ord2f)(const uint32_t* x, float* r, int64_t n, void* stream) { PROBE_MAP(k_ord2f, n, stream, x, r, n); }
/* L2, tol, cmax f32[n]; w, x, y f32[n,3]; nr i32[n] -> lo, cnt i32[n]; n < 2^29 */
int PN(bv_arc)(const float* L2, const float* w, const float* x, const float* y, const float* tol, const int* nr, const float* cmax,
               int* lo, int* cnt, int64_t n, void* stream)
{
    if (n >= ((int64_t)1 << 29)) return (int)hipErrorInvalidValue;
    PROBE_MAP(k_bv_arc, n, stream, L2, w, x, y, tol, nr, cmax, lo, cnt, n);
}

/* n a positive multiple of 256 (whole workgroups: the helpers are defined for full waves) */
int PN(wave_incl_scan)(const int* v, int* r, int64_t n, void* stream)
{
    if (n <= 0 || n % PROBE_THREADS || n / PROBE_THREADS > 65536) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wave_incl_scan, dim3((unsigned)(n / PROBE_THREADS)), dim3(PROBE_THREADS), 0, (hipStream_t)stream, v, r);
    CPPF_CHECK_LAUNCH();
    return 0;
}
int PN(wave_max_u64)(const unsigned long long* v, unsigned long long* r, int64_t n, void* stream)
{
    if (n <= 0 || n % PROBE_THREADS || n / PROBE_THREADS > 65536) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wave_max_u64, dim3((unsigned)(n / PROBE_THREADS)), dim3(PROBE_THREADS), 0, (hipStream_t)stream, v, r);
    CPPF_CHECK_LAUNCH();
    return 0;
}

/* out: device u64[2] = {mismatches, smallest mismatching operand (all ones: none)}; first + count <= 2^32 */
int PN(sweep_sqrt_rn)(uint32_t first, uint64_t count, unsigned long long* out, void* stream)
{
    if ((uint64_t)first + count > ((uint64_t)1 << 32)) return (int)hipErrorInvalidValue;
    if (int e = sweep_begin(out, (hipStream_t)stream)) return e;
    hipLaunchKernelGGL(k_sweep_sqrt, dim3(PROBE_SWEEP_BLOCKS), dim3(PROBE_THREADS), 0, (hipStream_t)stream, first, count, out);
    CPPF_CHECK_LAUNCH();
    return 0;
}
int PN(sweep_inv_sqrt_rn)(uint32_t first, uint64_t count, unsigned long long* out, void* stream)
{
    if ((uint64_t)first + count > ((uint64_t)1 << 32)) return (int)hipErrorInvalidValue;
    if (int e = sweep_begin(out, (hipStream_t)stream)) return e;
    hipLaunchKernelGGL(k_sweep_inv_sqrt, dim3(PROBE_SWEEP_BLOCKS), dim3(PROBE_THREADS), 0, (hipStream_t)stream, first, count, out);
    CPPF_CHECK_LAUNCH();
    return 0;
}
int PN(sweep_div_by)(float b, uint32_t first, uint64_t count, unsigned long long* out, void* stream)
{
    if ((uint64_t)first + count > ((uint64_t)1 << 31)) return (int)hipErrorInvalidValue;      /* magnitudes: both signs are tried */
    if (int e = sweep_begin(out, (hipStream_t)stream)) return e;
    hipLaunchKernelGGL(k_sweep_div, dim3(PROBE_SWEEP_BLOCKS), dim3(PROBE_THREADS), 0, (hipStream_t)stream, b, first, count, out);
    CPPF_CHECK_LAUNCH();
    return 0;
}
/* n_ratio: a power of two, 1 .. 65536 */
int PN(sweep_div_ppf)(uint32_t first, uint64_t count, int n_ratio, unsigned long long* out, void* stream)
{
    if ((uint64_t)first + count > ((uint64_t)1 << 31) || n_ratio < 1 || n_ratio > 65536 || (n_ratio & (n_ratio - 1))) return (int)hipErrorInvalidValue;
    if (int e = sweep_begin(out, (hipStream_t)stream)) return e;
    hipLaunchKernelGGL(k_sweep_div_ppf, dim3(PROBE_SWEEP_BLOCKS), dim3(PROBE_THREADS), 0, (hipStream_t)stream, first, count, n_ratio, out);
    CPPF_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
