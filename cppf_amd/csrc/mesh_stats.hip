// Voting statistics of a mesh category on gfx950 (MI355X): the body of the reference's gen_stats.py for a batch of meshes.
// C ABI, the arithmetic to the operation and the stated orders: include/cppf.h ("Mesh statistics").  The numpy restatement the
// tests hold these kernels to, bit for bit: tests/mesh_stats_ref.py.
//
// cppf_surface_sample_batch (Open3D's SamplePointsUniformly, area-weighted):
//   ms_area_kernel    one lane per face (all meshes): fp64 triangle area; a face index outside its mesh -> NaN + status bit 2
//   ms_sum_kernel     one 1024-lane workgroup per mesh: total area S in the blocked order of cppf.h; S not in (0, inf) -> bit 1
//   ms_norm_kernel    one lane per face: q_t = a_t / S
//   ms_scan_kernel    one 1024-lane workgroup per mesh: the cumulative q (blocked order), E_t = min(N, round(C_t N)), E_last = N,
//                     stored as its running maximum (E can step down by one behind a block boundary)
//   ms_points_kernel  one lane per point: its face (the first t with E_t > k: a bisection of the running maximum), two Philox
//                     uniforms, the barycentric point
// cppf_mesh_vote_stats_batch (generate_target's targets_tr and the maxima of gen_stats.py):
//   ms_bbox_kernel    one workgroup per mesh: bounding box, centre, diagonal, half extents (non-finite points -> status, NaN row)
//   ms_pairs_kernel   workgroups x meshes: Philox pairs, the per-pair fp64 arithmetic, per-workgroup maxima
//   ms_final_kernel   one lane per mesh: the maxima over workgroups, cast to float32
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"
#include "cppf_math.h"

#define MS_SCAN_THREADS 1024          // lanes of the per-mesh sum / scan workgroups: the block count of the stated order
#define MS_THREADS 256

static inline size_t ms_align(size_t b) { return (b + 255) & ~(size_t)255; }

// uniform double in [0, 1) from two words: the top 27 bits of w0 and the top 26 of w1 (53 bits), times 2^-53
__device__ __forceinline__ double ms_u53(unsigned w0, unsigned w1)
{
    const unsigned long long m = ((unsigned long long)(w0 >> 5) << 26) | (unsigned long long)(w1 >> 6);
    return (double)m * 0x1p-53;
}

// the mesh that owns global element g: the last m with off[m] <= g (off non-decreasing, off[0] = 0 <= g < off[M])
__device__ __forceinline__ int ms_owner(const int64_t* __restrict__ off, int M, int64_t g)
{
    int lo = 0, hi = M - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ surface sampling
struct MsSampleLayout { size_t voff, foff, area, E, S, total; };
static MsSampleLayout ms_sample_layout(int M, int64_t n_faces_total)
{
    MsSampleLayout L;
    size_t o = 0;
    L.voff = o; o += ms_align((size_t)(M + 1) * sizeof(int64_t));
    L.foff = o; o += ms_align((size_t)(M + 1) * sizeof(int64_t));
    L.area = o; o += ms_align((size_t)n_faces_total * sizeof(double));
    L.E = o;    o += ms_align((size_t)n_faces_total * sizeof(int32_t));
    L.S = o;    o += ms_align((size_t)M * sizeof(double));
    L.total = o;
    return L;
}

__global__ __launch_bounds__(MS_THREADS) void ms_area_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                             const int64_t* __restrict__ voff, const int64_t* __restrict__ foff, int M,
                                                             int64_t n_faces_total, double* __restrict__ area, int32_t* __restrict__ status)
{
    for (int64_t g = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; g < n_faces_total; g += (int64_t)gridDim.x * MS_THREADS) {
        const int m = ms_owner(foff, M, g);
        const int64_t v0 = voff[m], nv = voff[m + 1] - v0;
        const int32_t i0 = faces[3 * g], i1 = faces[3 * g + 1], i2 = faces[3 * g + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
            area[g] = __longlong_as_double(0x7ff8000000000000ll);
            atomicOr(&status[m], 2);
            continue;
        }
        const double* p0 = verts + 3 * (v0 + i0);
        const double* p1 = verts + 3 * (v0 + i1);
        const double* p2 = verts + 3 * (v0 + i2);
        const double x0 = p0[0] - p1[0], x1 = p0[1] - p1[1], x2 = p0[2] - p1[2];     // x = v0 - v1
        const double y0 = p0[0] - p2[0], y1 = p0[1] - p2[1], y2 = p0[2] - p2[2];     // y = v0 - v2
        const double c0 = x1 * y2 - x2 * y1, c1 = x2 * y0 - x0 * y2, c2 = x0 * y1 - x1 * y0;
        area[g] = 0.5 * sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    }
}

// lane l of the mesh's workgroup owns faces [l K, min(F, (l+1) K)), K = ceil(F / 1024)
__device__ __forceinline__ void ms_chunk(int64_t F, int64_t& t0, int64_t& t1)
{
    const int64_t K = (F + MS_SCAN_THREADS - 1) / MS_SCAN_THREADS;
    t0 = min(F, (int64_t)threadIdx.x * K);
    t1 = min(F, t0 + K);
}

// S = ((0 + s_0) + s_1) + ... + s_1023, s_l = ((0 + a_t0) + a_t0+1) + ...: lane sums left to right, lane totals in lane order
__global__ __launch_bounds__(MS_SCAN_THREADS) void ms_sum_kernel(const double* __restrict__ area, const int64_t* __restrict__ foff,
                                                                 double* __restrict__ S, int32_t* __restrict__ status)
{
    __shared__ double part[MS_SCAN_THREADS];
    const int m = blockIdx.x;
    const int64_t f0 = foff[m], F = foff[m + 1] - f0;
    int64_t t0, t1;
    ms_chunk(F, t0, t1);
    double s = 0.0;
    for (int64_t t = t0; t < t1; ++t) s = s + area[f0 + t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int l = 0; l < MS_SCAN_THREADS; ++l) tot = tot + part[l];
        S[m] = tot;
        if (!(tot > 0.0 && tot < INFINITY)) status[m] |= 1;
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_norm_kernel(double* __restrict__ area, const int64_t* __restrict__ foff, int M,
                                                             int64_t n_faces_total, const double* __restrict__ S)
{
    for (int64_t g = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; g < n_faces_total; g += (int64_t)gridDim.x * MS_THREADS)
        area[g] = area[g] / S[ms_owner(foff, M, g)];
}

// T_l = ((0 + q_t0) + q_t0+1) + ...;  B_0 = 0, B_l = B_l-1 + T_l-1;  C_t = (((B_l + q_t0) + q_t0+1) + ...) + q_t
__global__ __launch_bounds__(MS_SCAN_THREADS) void ms_scan_kernel(const double* __restrict__ q, const int64_t* __restrict__ foff,
                                                                  int64_t N, const int32_t* __restrict__ status, int32_t* __restrict__ E)
{
    __shared__ double part[MS_SCAN_THREADS];
    __shared__ int32_t top[MS_SCAN_THREADS];
    const int m = blockIdx.x;
    if (status[m] != 0) return;
    const int64_t f0 = foff[m], F = foff[m + 1] - f0;
    int64_t t0, t1;
    ms_chunk(F, t0, t1);
    double s = 0.0;
    for (int64_t t = t0; t < t1; ++t) s = s + q[f0 + t];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0.0;
        for (int l = 0; l < MS_SCAN_THREADS; ++l) {
            const double T = part[l];
            part[l] = b;
            b = b + T;
        }
    }
    __syncthreads();
    const double dN = (double)N;
    double c = part[threadIdx.x];
    int32_t last = 0;
    for (int64_t t = t0; t < t1; ++t) {
        c = c + q[f0 + t];
        const double r = round(c * dN);                       // halves away from zero (std::round)
        last = t == F - 1 ? (int32_t)N : (int32_t)(r < dN ? r : dN);
        E[f0 + t] = last;
    }
    // What is stored is the running maximum of E, so that "the first t with E_t > k" is a bisection whatever it probes.  Inside a
    // block E never decreases (q >= 0), but B_l+1 can round below the last C of block l (summed from B_l, not from zero), and
    // the lower value stays for as long as zero-area faces follow, across blocks too.  So: the maximum over the blocks before
    // this one (a max scan of their last E; an empty block counts 0), raised into this block's leading entries.
    top[threadIdx.x] = last;
    __syncthreads();
    for (int s = 1; s < MS_SCAN_THREADS; s <<= 1) {
        const int32_t o = (int)threadIdx.x >= s ? top[threadIdx.x - s] : 0;
        __syncthreads();
        top[threadIdx.x] = max(top[threadIdx.x], o);
        __syncthreads();
    }
    const int32_t before = threadIdx.x > 0 ? top[threadIdx.x - 1] : 0;
    for (int64_t t = t0; t < t1 && E[f0 + t] < before; ++t) E[f0 + t] = before;
}

__global__ __launch_bounds__(MS_THREADS) void ms_points_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                               const int64_t* __restrict__ voff, const int64_t* __restrict__ foff,
                                                               const int32_t* __restrict__ E, const int32_t* __restrict__ status,
                                                               int64_t N, int64_t blocks_per_mesh, uint2 key, unsigned first_mesh,
                                                               double* __restrict__ points, int32_t* __restrict__ face_ids)
{
    const int m = (int)(blockIdx.x / blocks_per_mesh);
    const int64_t k = (int64_t)(blockIdx.x % blocks_per_mesh) * MS_THREADS + threadIdx.x;
    if (k >= N) return;
    const int64_t o = (int64_t)m * N + k;
    if (status[m] != 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        points[3 * o] = nan;
        points[3 * o + 1] = nan;
        points[3 * o + 2] = nan;
        if (face_ids) face_ids[o] = -1;
        return;
    }
    const int64_t f0 = foff[m];
    int64_t lo = 0, hi = foff[m + 1] - f0 - 1;                // the first face t with E_t > k (E_last = N > k); E holds the running
                                                              // maximum, so "E > k" is false, then true, wherever mid falls
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (E[f0 + mid] > k) hi = mid; else lo = mid + 1;
    }
    const int64_t g = f0 + lo, v0 = voff[m];
    const double* p0 = verts + 3 * (v0 + faces[3 * g]);
    const double* p1 = verts + 3 * (v0 + faces[3 * g + 1]);
    const double* p2 = verts + 3 * (v0 + faces[3 * g + 2]);
    const uint4 w = philox4x32_10(make_uint4((unsigned)k, first_mesh + (unsigned)m, 2u, 0u), key);
    const double r1 = ms_u53(w.x, w.y), r2 = ms_u53(w.z, w.w);
    const double s = sqrt(r1);
    const double a = 1.0 - s, b = s * (1.0 - r2), c = s * r2;
#pragma unroll
    for (int j = 0; j < 3; ++j) points[3 * o + j] = (a * p0[j] + b * p1[j]) + c * p2[j];
    if (face_ids) face_ids[o] = (int32_t)lo;
}

extern "C" size_t cppf_surface_sample_workspace_bytes(int n_meshes, int64_t n_faces_total)
{
    if (n_meshes < 1 || n_faces_total < n_meshes) return 0;
    return ms_sample_layout(n_meshes, n_faces_total).total;
}

extern "C" int cppf_surface_sample_batch(const double* verts, const int32_t* faces, const int64_t* vert_off_host,
                                         const int64_t* face_off_host, int n_meshes, int64_t n_points, unsigned long long seed,
                                         int64_t first_mesh, double* points, int32_t* face_ids, int32_t* status, void* workspace,
                                         size_t workspace_bytes, void* stream)
{
    if (!verts || !faces || !vert_off_host || !face_off_host || !points || !status || n_meshes < 1 || n_points < 1 ||
        n_points > 0x7fffffffll || first_mesh < 0 || first_mesh + n_meshes > 0x100000000ll)
        return CPPF_EINVAL;
    if (vert_off_host[0] != 0 || face_off_host[0] != 0) return CPPF_EINVAL;
    for (int m = 0; m < n_meshes; ++m) {
        const int64_t nf = face_off_host[m + 1] - face_off_host[m], nv = vert_off_host[m + 1] - vert_off_host[m];
        if (nf < 1 || nf > 0x7fffffffll || nv < 1 || nv > 0x7fffffffll) return CPPF_EINVAL;
    }
    const int64_t n_faces_total = face_off_host[n_meshes];
    const int64_t bpm = (n_points + MS_THREADS - 1) / MS_THREADS;
    if (bpm * n_meshes > 0x7fffffffll) return CPPF_EINVAL;
    const MsSampleLayout L = ms_sample_layout(n_meshes, n_faces_total);
    if (!workspace || workspace_bytes < L.total) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    int64_t* voff = reinterpret_cast<int64_t*>(ws + L.voff);
    int64_t* foff = reinterpret_cast<int64_t*>(ws + L.foff);
    double* area = reinterpret_cast<double*>(ws + L.area);
    int32_t* E = reinterpret_cast<int32_t*>(ws + L.E);
    double* S = reinterpret_cast<double*>(ws + L.S);
    const size_t ob = (size_t)(n_meshes + 1) * sizeof(int64_t);
    hipError_t e = hipMemcpyAsync(voff, vert_off_host, ob, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(foff, face_off_host, ob, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)n_meshes * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const int64_t nfb = (n_faces_total + MS_THREADS - 1) / MS_THREADS;
    // at most 8192 workgroups of 256 lanes a trip (tested: 2 100 000 faces in two meshes, the second one on both sides of face
    // 2 097 152: tests/test_gpu_mesh_stats_edges.py)
    const unsigned gf = (unsigned)(nfb < 8192 ? nfb : 8192);
    ms_area_kernel<<<gf, MS_THREADS, 0, st>>>(verts, faces, voff, foff, n_meshes, n_faces_total, area, status);
    ms_sum_kernel<<<n_meshes, MS_SCAN_THREADS, 0, st>>>(area, foff, S, status);
    ms_norm_kernel<<<gf, MS_THREADS, 0, st>>>(area, foff, n_meshes, n_faces_total, S);
    ms_scan_kernel<<<n_meshes, MS_SCAN_THREADS, 0, st>>>(area, foff, n_points, status, E);
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    ms_points_kernel<<<(unsigned)(bpm * n_meshes), MS_THREADS, 0, st>>>(verts, faces, voff, foff, E, status, n_points, bpm, key,
                                                                         (unsigned)first_mesh, points, face_ids);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ vote statistics
#define MS_PAIR_BLOCKS_TARGET 4096    // workgroups of one ms_pairs_kernel launch, about (>= 16 per CU), when the pairs allow
                                      // (tested: three trips of 8 workgroups x 512 meshes, four of 14 x 300 and three of 4096 x 1,
                                      // each with a ragged last trip and maxima in the later trips: tests/test_gpu_mesh_stats_edges.py)

static int64_t ms_pair_blocks(int M, int64_t P)
{
    const int64_t need = (P + MS_THREADS - 1) / MS_THREADS;
    const int64_t want = (MS_PAIR_BLOCKS_TARGET + M - 1) / M;
    return need < want ? need : want;
}

struct MsStatsLayout { size_t centre, part, total; };
static MsStatsLayout ms_stats_layout(int M, int64_t P)
{
    MsStatsLayout L;
    size_t o = 0;
    L.centre = o; o += ms_align((size_t)M * 3 * sizeof(double));
    L.part = o;   o += ms_align((size_t)M * (size_t)ms_pair_blocks(M, P) * 2 * sizeof(double));
    L.total = o;
    return L;
}

__global__ __launch_bounds__(MS_THREADS) void ms_bbox_kernel(const double* __restrict__ pts, int64_t N, double* __restrict__ centre,
                                                             double* __restrict__ stats, int32_t* __restrict__ status)
{
    __shared__ double slo[3][MS_THREADS], shi[3][MS_THREADS];
    __shared__ int sbad[MS_THREADS];
    const int m = blockIdx.x;
    const double* p = pts + (int64_t)m * N * 3;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int64_t i = threadIdx.x; i < N; i += MS_THREADS)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v = p[3 * i + j];
            bad |= !isfinite(v);
            lo[j] = fmin(lo[j], v);
            hi[j] = fmax(hi[j], v);
        }
#pragma unroll
    for (int j = 0; j < 3; ++j) { slo[j][threadIdx.x] = lo[j]; shi[j][threadIdx.x] = hi[j]; }
    sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = MS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                slo[j][threadIdx.x] = fmin(slo[j][threadIdx.x], slo[j][threadIdx.x + s]);
                shi[j][threadIdx.x] = fmax(shi[j][threadIdx.x], shi[j][threadIdx.x + s]);
            }
            sbad[threadIdx.x] |= sbad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* row = stats + 6 * (int64_t)m;
    if (sbad[0]) {
        status[m] = 1;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int j = 0; j < 6; ++j) row[j] = nan;
        return;
    }
    status[m] = 0;
    double ext[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double c = (slo[j][0] + shi[j][0]) / 2.0;
        const double hc = shi[j][0] - c, lc = slo[j][0] - c;     // max / min of the centred points (rounding is monotonic)
        centre[3 * m + j] = c;
        ext[j] = hc - lc;
        row[3 + j] = hc;
    }
    row[0] = sqrt((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]);
}

__global__ __launch_bounds__(MS_THREADS) void ms_pairs_kernel(const double* __restrict__ pts, int64_t N, int64_t P, int64_t nb,
                                                              uint2 key, unsigned first_mesh, const double* __restrict__ centre,
                                                              const int32_t* __restrict__ status, double* __restrict__ part)
{
    __shared__ double sp[MS_THREADS], sd[MS_THREADS];
    const int m = (int)(blockIdx.x / nb);
    const int64_t b = blockIdx.x % nb;
    if (status[m] != 0) return;
    const double* p = pts + (int64_t)m * N * 3;
    const double cx = centre[3 * m], cy = centre[3 * m + 1], cz = centre[3 * m + 2];
    const unsigned long long n = (unsigned long long)N;
    double mp = 0.0, md = 0.0;
    for (int64_t q = b * MS_THREADS + threadIdx.x; q < P; q += nb * MS_THREADS) {
        const uint4 w = philox4x32_10(make_uint4((unsigned)q, first_mesh + (unsigned)m, 3u, 0u), key);
        const int64_t i = (int64_t)(((unsigned long long)w.x * n) >> 32), j = (int64_t)(((unsigned long long)w.y * n) >> 32);
        const double ax = p[3 * i] - cx, ay = p[3 * i + 1] - cy, az = p[3 * i + 2] - cz;
        const double bx = p[3 * j] - cx, by = p[3 * j + 1] - cy, bz = p[3 * j + 2] - cz;
        const double dx = ax - bx, dy = ay - by, dz = az - bz;
        const double den = sqrt((dx * dx + dy * dy) + dz * dz) + 1e-7;
        const double ux = dx / den, uy = dy / den, uz = dz / den;
        const double proj = (ax * ux + ay * uy) + az * uz;
        const double ox = ax - proj * ux, oy = ay - proj * uy, oz = az - proj * uz;
        const double dist2o = sqrt((ox * ox + oy * oy) + oz * oz);
        mp = fmax(mp, fabs(proj));
        md = fmax(md, dist2o);
    }
    sp[threadIdx.x] = mp;
    sd[threadIdx.x] = md;
    __syncthreads();
    for (int s = MS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sp[threadIdx.x] = fmax(sp[threadIdx.x], sp[threadIdx.x + s]);
            sd[threadIdx.x] = fmax(sd[threadIdx.x], sd[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sp[0];
        part[2 * blockIdx.x + 1] = sd[0];
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_final_kernel(const double* __restrict__ part, int M, int64_t nb,
                                                              const int32_t* __restrict__ status, double* __restrict__ stats)
{
    const int m = blockIdx.x * MS_THREADS + threadIdx.x;
    if (m >= M || status[m] != 0) return;
    double mp = 0.0, md = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
        mp = fmax(mp, part[2 * (m * nb + b)]);
        md = fmax(md, part[2 * (m * nb + b) + 1]);
    }
    stats[6 * (int64_t)m + 1] = (double)(float)mp;
    stats[6 * (int64_t)m + 2] = (double)(float)md;
}

extern "C" size_t cppf_mesh_vote_stats_workspace_bytes(int n_meshes, int64_t n_points, int64_t n_pairs)
{
    if (n_meshes < 1 || n_points < 1 || n_pairs < 1 || n_pairs > 0xffffffffll) return 0;
    return ms_stats_layout(n_meshes, n_pairs).total;
}

extern "C" int cppf_mesh_vote_stats_batch(const double* points, int n_meshes, int64_t n_points, int64_t n_pairs, unsigned long long seed,
                                          int64_t first_mesh, double* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                                          void* stream)
{
    if (!points || !stats || !status || n_meshes < 1 || n_points < 1 || n_points > 0x7fffffffll || n_pairs < 1 ||
        n_pairs > 0xffffffffll || first_mesh < 0 || first_mesh + n_meshes > 0x100000000ll)
        return CPPF_EINVAL;
    const int64_t nb = ms_pair_blocks(n_meshes, n_pairs);
    if (nb * n_meshes > 0x7fffffffll) return CPPF_EINVAL;
    const MsStatsLayout L = ms_stats_layout(n_meshes, n_pairs);
    if (!workspace || workspace_bytes < L.total) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    double* centre = reinterpret_cast<double*>(ws + L.centre);
    double* part = reinterpret_cast<double*>(ws + L.part);
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    ms_bbox_kernel<<<n_meshes, MS_THREADS, 0, st>>>(points, n_points, centre, stats, status);
    ms_pairs_kernel<<<(unsigned)(nb * n_meshes), MS_THREADS, 0, st>>>(points, n_points, n_pairs, nb, key, (unsigned)first_mesh, centre,
                                                                     status, part);
    ms_final_kernel<<<(n_meshes + MS_THREADS - 1) / MS_THREADS, MS_THREADS, 0, st>>>(part, n_meshes, nb, status, stats);
    return (int)hipGetLastError();
}
