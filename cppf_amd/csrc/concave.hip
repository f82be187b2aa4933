// Concave creases of a depth frame for gfx950 (MI355X): a local plane fit per pixel, and the pixels across which two fitted surfaces
// turn TOWARDS each other -- where an object stands on its support or leans on a neighbour.  The mask goes into cppf_depth_segments
// as `valid` (cppf_amd/segments.py: frame_segments(concave=)).  C ABI and the definitions: include/cppf.h ("Concave edges");
// restated in numpy: tests/concave_ref.py; DESIGN.md 3.7l.
//
// cppf_concave_edges, three launches, no workspace -- `normal` carries the fit between them:
//   cc_fit_kernel     one workgroup of 256 lanes per 32 x 8 pixel tile.  The tile and its halo of `radius` go into LDS once as u16
//                     with dead and out-of-frame pixels stored as 0 (`valid` and the frame test folded in; <= 48 x 24 x 2 B).  A lane
//                     walks its (2r+1)^2 window out of LDS with the nine sums in 32-bit registers (exact: the caps keep every sum
//                     under 2^31), takes the four Cramer determinants in int64 (exact, under 2^53) and makes THREE fp64 divisions.
//                     normal[p] <- {c, a, b}: the fitted depth in metres and its two slopes in metres per pixel, {0, 0, 0} without
//                     a fit.  counts <- 0.
//   cc_edge_kernel    one lane per pixel: the surfaces {N, P} of the four pixels at +-step are derived from their {c, a, b}
//                     (cc_surface: the one body the definition's fp64 order lives in), the three tests per axis, edge[p]; one
//                     ballot-counted integer add per wave for the edge and the live pixels.  normal is read-only here.
//   cc_normal_kernel  normal[p] <- the unit normal of its own {c, a, b} (zeros without a fit), in place: every lane its own three
//                     words, after the kernel boundary that ends all reads of them; the fits are counted by ballot.
// Integer atomics only, vector stores only, no allocation, no host synchronisation: the call can be captured in a graph and gives
// the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"

#define CC_BLOCK 256
#define CC_TW 32
#define CC_TH 8
#define CC_RMAX CPPF_CONCAVE_MAX_RADIUS
#define CC_SMAX CPPF_CONCAVE_MAX_STEP
#define CC_LW (CC_TW + 2 * CC_RMAX)
#define CC_LH (CC_TH + 2 * CC_RMAX)
#define CC_MAX_PIXELS (1 << 24)

struct CcCam {
    double fx, fy, cx, cy;
};

struct CcSurface {
    double nx, ny, nz, px, py, pz;
    bool fit;
};

// include/cppf.h "Concave edges", steps 4-6: every line one rounding per operation, in this order (-ffp-contract=off)
__device__ __forceinline__ CcSurface cc_surface(double c, double am, double bm, int u, int v, const CcCam k)
{
    const double xu = (double)u - k.cx, yv = (double)v - k.cy;
    const double pux = c / k.fx + (xu * am) / k.fx, puy = (yv * am) / k.fy, puz = am;
    const double pvx = (xu * bm) / k.fx, pvy = c / k.fy + (yv * bm) / k.fy, pvz = bm;
    double nx = puy * pvz - puz * pvy, ny = puz * pvx - pux * pvz, nz = pux * pvy - puy * pvx;
    CcSurface s;
    s.px = (xu * c) / k.fx;
    s.py = (yv * c) / k.fy;
    s.pz = c;
    if ((nx * s.px + ny * s.py) + nz * s.pz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double ln = sqrt((nx * nx + ny * ny) + nz * nz);
    s.fit = isfinite(ln) && ln > 0.0;
    s.nx = s.fit ? nx / ln : 0.0;
    s.ny = s.fit ? ny / ln : 0.0;
    s.nz = s.fit ? nz / ln : 0.0;
    return s;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_fit_kernel(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ valid, int H, int W,
                                                          int tiles_x, int r, int tol, int slope, int min_count,
                                                          double* __restrict__ abc, int32_t* __restrict__ counts)
{
    __shared__ uint16_t s_z[CC_LH * CC_LW];
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && t < 4) counts[t] = 0;
    // the tiles are numbered along ONE grid dimension: a frame of one column has more tile rows than a second dimension takes
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * CC_TW - r, y0 = by * CC_TH - r;
    const int lw = CC_TW + 2 * r, lh = CC_TH + 2 * r;
    for (int i = t; i < lw * lh; i += CC_BLOCK) {
        const int ly = i / lw, lx = i - ly * lw;
        const int x = x0 + lx, y = y0 + ly;
        uint16_t z = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const int p = y * W + x;                                           // H * W <= 2^24
            z = depth[p];
            if (valid && !valid[p]) z = 0;
        }
        s_z[ly * CC_LW + lx] = z;
    }
    __syncthreads();
    const int tx = t & (CC_TW - 1), ty = t / CC_TW;
    const int x = bx * CC_TW + tx, y = by * CC_TH + ty;
    if (x >= W || y >= H) return;
    const uint16_t* win = s_z + (ty + r) * CC_LW + (tx + r);                   // the centre; offsets -r..r stay inside the staged tile
    const int z0 = win[0];
    double c = 0.0, am = 0.0, bm = 0.0;
    if (z0 > 0) {
        const int lim = tol + (slope * z0) / 1000;                             // <= 65535 + 65535
        int n = 0, su = 0, sv = 0, suu = 0, suv = 0, svv = 0, sz = 0, szu = 0, szv = 0;
        for (int dv = -r; dv <= r; ++dv) {
            const int adv = dv < 0 ? -dv : dv;
            for (int du = -r; du <= r; ++du) {
                const int zq = win[dv * CC_LW + du];
                const int adu = du < 0 ? -du : du;
                const int m = adu > adv ? adu : adv;
                const int dz = zq - z0;
                const int adz = dz < 0 ? -dz : dz;
                if (zq > 0 && adz <= lim * (m > 1 ? m : 1)) {                  // lim * 8 < 2^21
                    n += 1; su += du; sv += dv; suu += du * du; suv += du * dv; svv += dv * dv;
                    sz += dz; szu += dz * du; szv += dz * dv;                   // |dz| <= 65535: |szu| <= 1224 * 65535 < 2^27
                }
            }
        }
        if (n >= min_count) {
            const int64_t N = n, Su = su, Sv = sv, Suu = suu, Suv = suv, Svv = svv, Sz = sz, Szu = szu, Szv = szv;
            const int64_t C00 = Suu * Svv - Suv * Suv, C01 = Suv * Sv - Su * Svv, C02 = Su * Suv - Suu * Sv;
            const int64_t C11 = N * Svv - Sv * Sv, C12 = Su * Sv - N * Suv, C22 = N * Suu - Su * Su;
            const int64_t D = N * C00 + Su * C01 + Sv * C02;
            if (D > 0) {
                const double d = (double)D;                                    // every determinant is under 2^53: the conversions are exact
                const double c0 = (double)(C00 * Sz + C01 * Szu + C02 * Szv) / d;
                const double a = (double)(C01 * Sz + C11 * Szu + C12 * Szv) / d;
                const double b = (double)(C02 * Sz + C12 * Szu + C22 * Szv) / d;
                c = ((double)z0 + c0) / 1000.0;
                am = a / 1000.0;
                bm = b / 1000.0;
            }
        }
    }
    double* o = abc + 3 * (int64_t)(y * W + x);
    o[0] = c;
    o[1] = am;
    o[2] = bm;
}

__device__ __forceinline__ CcSurface cc_surface_at(const double* __restrict__ abc, int W, int u, int v, const CcCam k)
{
    const double* q = abc + 3 * (int64_t)(v * W + u);
    return cc_surface(q[0], q[1], q[2], u, v, k);
}

__device__ __forceinline__ bool cc_concave(const CcSurface m, const CcSurface p, double span2_max, double cos_max)
{
    if (!m.fit || !p.fit) return false;
    const double dx = p.px - m.px, dy = p.py - m.py, dz = p.pz - m.pz;
    const double ex = p.nx - m.nx, ey = p.ny - m.ny, ez = p.nz - m.nz;
    const double span2 = (dx * dx + dy * dy) + dz * dz;
    const double cosn = (m.nx * p.nx + m.ny * p.ny) + m.nz * p.nz;
    const double conv = (dx * ex + dy * ey) + dz * ez;
    return span2 <= span2_max && cosn < cos_max && conv < 0.0;
}

__global__ __launch_bounds__(CC_BLOCK) void cc_edge_kernel(const uint16_t* __restrict__ depth, const uint8_t* __restrict__ valid, int H, int W,
                                                           int s, CcCam k, double span2_max, double cos_max, const double* __restrict__ abc,
                                                           uint8_t* __restrict__ edge, int32_t* counts)
{
    const int n = H * W;
    const int p = blockIdx.x * CC_BLOCK + threadIdx.x;
    const bool in = p < n;
    const bool live = in && depth[p] > 0 && (!valid || valid[p]);
    bool mark = false;
    if (live) {
        const int v = p / W, u = p - v * W;
        if (u - s >= 0 && u + s < W) mark = cc_concave(cc_surface_at(abc, W, u - s, v, k), cc_surface_at(abc, W, u + s, v, k), span2_max, cos_max);
        if (!mark && v - s >= 0 && v + s < H)
            mark = cc_concave(cc_surface_at(abc, W, u, v - s, k), cc_surface_at(abc, W, u, v + s, k), span2_max, cos_max);
    }
    if (in) edge[p] = mark ? 1 : 0;
    const unsigned long long m_live = __ballot(live), m_mark = __ballot(mark);
    if ((threadIdx.x & 63) == 0) {
        if (m_mark) atomicAdd(counts + 0, __popcll(m_mark));
        if (m_live) atomicAdd(counts + 2, __popcll(m_live));
    }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_normal_kernel(int H, int W, CcCam k, double* normal, int32_t* counts)
{
    const int n = H * W;
    const int p = blockIdx.x * CC_BLOCK + threadIdx.x;
    bool fit = false;
    if (p < n) {
        const int v = p / W, u = p - v * W;
        double* q = normal + 3 * (int64_t)p;
        const CcSurface s = cc_surface(q[0], q[1], q[2], u, v, k);
        fit = s.fit;
        q[0] = s.nx;
        q[1] = s.ny;
        q[2] = s.nz;
    }
    const unsigned long long m_fit = __ballot(fit);
    if ((threadIdx.x & 63) == 0 && m_fit) atomicAdd(counts + 1, __popcll(m_fit));
}

extern "C" int cppf_concave_edges(const int16_t* depth, const uint8_t* valid, int H, int W, double fx, double fy, double cx, double cy,
                                  int radius, int step, int tol_mm, int slope_permille, int min_count, double cos_max, double span_max,
                                  uint8_t* edge, double* normal, int32_t* counts, void* stream)
{
    if (H < 1 || W < 1 || (int64_t)H * W > CC_MAX_PIXELS) return CPPF_EINVAL;
    if (radius < 1 || radius > CC_RMAX || step < 1 || step > CC_SMAX) return CPPF_EINVAL;
    if (tol_mm < 0 || tol_mm > 65535 || slope_permille < 0 || slope_permille > 1000 || min_count < 3) return CPPF_EINVAL;
    if (!(cos_max > -1.0 && cos_max < 1.0) || !(span_max > 0.0) || !isfinite(span_max)) return CPPF_EINVAL;
    if (!(fx > 0.0) || !(fy > 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return CPPF_EINVAL;
    if (!depth || !edge || !normal || !counts) return CPPF_EINVAL;
    const int n = H * W;
    const CcCam k = {fx, fy, cx, cy};
    const uint16_t* d = (const uint16_t*)depth;
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (W + CC_TW - 1) / CC_TW, tiles_y = (H + CC_TH - 1) / CC_TH;      // tiles_x * tiles_y <= 2^24 / 256 + 2^24 / 32 + 2^24 / 8 + 1
    const dim3 tiles((unsigned)(tiles_x * tiles_y)), flat((unsigned)((n + CC_BLOCK - 1) / CC_BLOCK));
    hipLaunchKernelGGL(cc_fit_kernel, tiles, dim3(CC_BLOCK), 0, s, d, valid, H, W, tiles_x, radius, tol_mm, slope_permille, min_count, normal,
                       counts);
    hipLaunchKernelGGL(cc_edge_kernel, flat, dim3(CC_BLOCK), 0, s, d, valid, H, W, step, k, span_max * span_max, cos_max,
                       (const double*)normal, edge, counts);
    hipLaunchKernelGGL(cc_normal_kernel, flat, dim3(CC_BLOCK), 0, s, H, W, k, normal, counts);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}
