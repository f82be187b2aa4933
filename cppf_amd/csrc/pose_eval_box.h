// The oriented-box IoU of cppf_amd/evaluation.py (_frame, _clip, _flux, box_intersection_volume, _iou_frames) as device functions:
// shared by csrc/pose_eval.hip (cppf_pose_eval_pairs) and csrc/box_nms.hip (cppf_box_nms_batch), so that both compute the same bits.
// All arithmetic is fp64 in evaluation.py's order, without contraction (-ffp-contract=off).  A caller gives every lane its own
// polygon slots in LDS: double poly[2 * PE_MAXV * 3 * PE_LANES], buf = poly + lane (a workgroup is one wavefront of PE_LANES lanes).
#ifndef CPPF_POSE_EVAL_BOX_H
#define CPPF_POSE_EVAL_BOX_H
#include <hip/hip_runtime.h>
#include <math.h>

#define PE_LANES 64            // lanes of a pe_pairs_kernel workgroup (one wavefront)
#define PE_MAXV 10             // vertices of a quad after six half-space cuts, at most

// ------------------------------------------------------------------------------------------------ oriented boxes
struct PeFrame { double c[3], U[3][3], h[3]; };          // centre, unit axes U[row][axis], half extents (evaluation._frame)

__device__ __forceinline__ double pe_det3(const double R[3][3])
{
    return (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0])) +
           R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
}

__device__ __forceinline__ void pe_frame(const double R_in[3][3], const double t[3], const double sc[3], PeFrame& f)
{
    const double s = cbrt(pe_det3(R_in));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double r0 = R_in[0][a] / s, r1 = R_in[1][a] / s, r2 = R_in[2][a] / s;
        const double nrm = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
        f.U[0][a] = r0 / nrm;
        f.U[1][a] = r1 / nrm;
        f.U[2][a] = r2 / nrm;
        f.h[a] = (0.5 * sc[a]) * nrm;
        f.c[a] = t[a];
    }
}

// evaluation._clip: the part of the polygon `src` (m vertices) inside n.x <= d, written to `dst`; returns its vertex count.
// src / dst are the lane's own slots: vertex v, coordinate c at [(v * 3 + c) * PE_LANES].  A convex polygon gains at most one
// vertex per cut; the store is bounded all the same, so that no rounding pattern can write outside the lane's slots.
__device__ __forceinline__ int pe_clip(const double* src, double* dst, int m, double n0, double n1, double n2, double d, double tol)
{
    double ax = src[0], ay = src[PE_LANES], az = src[2 * PE_LANES];
    double da = ((ax * n0 + ay * n1) + az * n2) - d;
    const double fx = ax, fy = ay, fz = az, df = da;
    int cnt = 0;
    for (int i = 0; i < m; ++i) {
        double bx = fx, by = fy, bz = fz, db = df;
        if (i + 1 < m) {
            const double* q = src + (i + 1) * 3 * PE_LANES;
            bx = q[0]; by = q[PE_LANES]; bz = q[2 * PE_LANES];
            db = ((bx * n0 + by * n1) + bz * n2) - d;
        }
        const bool ia = da <= tol, ib = db <= tol;
        if (ia) {
            if (cnt < PE_MAXV) {
                double* o = dst + cnt * 3 * PE_LANES;
                o[0] = ax; o[PE_LANES] = ay; o[2 * PE_LANES] = az;
            }
            ++cnt;
        }
        if (ia != ib) {
            const double t = fmin(1.0, fmax(0.0, da / (da - db)));
            if (cnt < PE_MAXV) {
                double* o = dst + cnt * 3 * PE_LANES;
                o[0] = ax + t * (bx - ax); o[PE_LANES] = ay + t * (by - ay); o[2 * PE_LANES] = az + t * (bz - az);
            }
            ++cnt;
        }
        ax = bx; ay = by; az = bz; da = db;
    }
    return cnt < PE_MAXV ? cnt : PE_MAXV;
}

// evaluation._flux: (n . x) * area of the planar polygon
__device__ __forceinline__ double pe_flux(const double* p, int m, double d)
{
    if (m < 3) return 0.0;
    const double x0 = p[0], y0 = p[PE_LANES], z0 = p[2 * PE_LANES];
    double ux = p[3 * PE_LANES] - x0, uy = p[4 * PE_LANES] - y0, uz = p[5 * PE_LANES] - z0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = 2; i < m; ++i) {
        const double* q = p + i * 3 * PE_LANES;
        const double vx = q[0] - x0, vy = q[PE_LANES] - y0, vz = q[2 * PE_LANES] - z0;
        sx += uy * vz - uz * vy;
        sy += uz * vx - ux * vz;
        sz += ux * vy - uy * vx;
        ux = vx; uy = vy; uz = vz;
    }
    return d * (0.5 * sqrt((sx * sx + sy * sy) + sz * sz));
}

// evaluation.box_intersection_volume: the faces of box A clipped by box B's closed half-spaces (+tol), then the faces of box B
// clipped by box A's open ones (-tol); a half-space facing against the clipped face's normal is open either way.
// buf: the lane's two polygon buffers, PE_MAXV * 3 * PE_LANES doubles apart.
__device__ __forceinline__ double pe_volume(PeFrame A, PeFrame B, double* buf)
{
    const double scale = fmax(fmax(fmax(A.h[0], A.h[1]), A.h[2]), fmax(fmax(B.h[0], B.h[1]), B.h[2]));
    double tol = 1e-9 * scale, total = 0.0;
#pragma unroll 1
    for (int dir = 0; dir < 2; ++dir) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int a = (k + 1) % 3, b = (k + 2) % 3;
#pragma unroll 1
            for (int si = 0; si < 2; ++si) {
                const double s = si ? -1.0 : 1.0;
                const double sh = s * A.h[k];
                double ctr[3], ea[3], eb[3], n[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    ctr[r] = A.c[r] + sh * A.U[r][k];
                    ea[r] = A.h[a] * A.U[r][a];
                    eb[r] = A.h[b] * A.U[r][b];
                    n[r] = s * A.U[r][k];
                }
                const double d = (n[0] * ctr[0] + n[1] * ctr[1]) + n[2] * ctr[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    buf[(0 * 3 + r) * PE_LANES] = (ctr[r] - ea[r]) - eb[r];
                    buf[(1 * 3 + r) * PE_LANES] = (ctr[r] + ea[r]) - eb[r];
                    buf[(2 * 3 + r) * PE_LANES] = (ctr[r] + ea[r]) + eb[r];
                    buf[(3 * 3 + r) * PE_LANES] = (ctr[r] - ea[r]) + eb[r];
                }
                int m = 4, cur = 0;
#pragma unroll
                for (int k2 = 0; k2 < 3; ++k2) {
#pragma unroll 1
                    for (int s2i = 0; s2i < 2; ++s2i) {
                        if (m < 3) continue;                       // (the host stops clipping here; the flux of < 3 vertices is 0)
                        const double s2 = s2i ? -1.0 : 1.0;
                        const double sh2 = s2 * B.h[k2];
                        const double n0 = s2 * B.U[0][k2], n1 = s2 * B.U[1][k2], n2 = s2 * B.U[2][k2];
                        const double c0 = B.c[0] + sh2 * B.U[0][k2], c1 = B.c[1] + sh2 * B.U[1][k2], c2 = B.c[2] + sh2 * B.U[2][k2];
                        const double d2 = (n0 * c0 + n1 * c1) + n2 * c2;
                        // a half-space that faces against this face's normal is open in both directions: boxes that touch from
                        // opposite sides of a plane share no volume, their common face is no face of the intersection
                        const bool against = (n[0] * n0 + n[1] * n1) + n[2] * n2 < 0.0;
                        m = pe_clip(buf + cur * (PE_MAXV * 3 * PE_LANES), buf + (cur ^ 1) * (PE_MAXV * 3 * PE_LANES), m, n0, n1, n2, d2,
                                    against ? -fabs(tol) : tol);
                        cur ^= 1;
                    }
                }
                total += pe_flux(buf + cur * (PE_MAXV * 3 * PE_LANES), m, d);
            }
        }
        const PeFrame T = A;
        A = B;
        B = T;
        tol = -tol;
    }
    return fmax(total / 3.0, 0.0);
}

// evaluation._iou_frames
__device__ __forceinline__ double pe_iou(const PeFrame& A, const PeFrame& B, double* buf)
{
    const double v = pe_volume(A, B, buf);
    const double va = 8.0 * ((A.h[0] * A.h[1]) * A.h[2]), vb = 8.0 * ((B.h[0] * B.h[1]) * B.h[2]);
    if (v <= 1e-9 * fmin(va, vb)) return 0.0;
    const double r = v / ((va + vb) - v);
    return r > 0.0 ? r : 0.0;
}

#endif  // CPPF_POSE_EVAL_BOX_H
