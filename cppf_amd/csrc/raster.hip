// Depth-only triangle rasteriser for gfx950 (MI355X): the training view of utils/dataset.py:103-201, the pyrender
// `RenderFlags.DEPTH_ONLY` render of one mesh through the dataset's PinholeCamera, and the compaction of the rendered pixels into
// the point cloud of :203-207.  C ABI, the arithmetic to the operation and the stated assumptions: include/cppf.h.  The numpy
// restatement the tests hold these kernels to, bit for bit: tests/mesh_ref.py.
//
//   rs_setup_kernel    one lane per triangle: fp64 model-view transform, near-plane clip (<= 2 primitives), projection, cull,
//                      edge set-up, conservative pixel bbox
//   rs_count_kernel    per primitive: +1 on every 16x16 screen tile its bbox touches
//   rs_scan_kernel     one workgroup: exclusive scan of the tile counts, the capacity check (status), the scatter cursors
//   rs_scatter_kernel  per primitive: its id into the bin list of every tile it touches
//   rs_raster_kernel   one workgroup per tile, one lane per pixel: every lane tests its own pixel centre against the tile's
//                      primitives (staged 256 at a time in LDS) and keeps the minimum depth in a register; one plain store
//   rs_points_kernel   cppf_depth_points: covered pixels -> fp64 points in row-major order (after cppf_compact_mask)
//
// cppf_raster_instances draws K posed instances of several meshes into ONE depth image with a label image, through the same
// device functions (rs_setup_face, rs_emit, the raster kernel's body) in one binned pass:
//   rs_inst_scan_kernel   one workgroup: prefix sums of the instances' face counts (item q -> instance by a search in them)
//   rs_setup_inst_kernel  one lane per instanced face q: finds its instance, reads that instance's matrix and mesh ranges from the
//                         workspace, then rs_setup_face; the instance index rides in the primitive record's spare bytes
//   rs_raster_kernel<true>  keeps (depth, instance) per lane; on equal depth the lowest instance index wins
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cppf.h"

#define RS_TILE 16                    // screen tiles of 16 x 16 pixels: one 256-lane workgroup each
#define RS_THREADS 256
#define RS_MAX_DIM 8192               // W, H <= 8192
#define RS_MAX_INST 65536             // instances of one cppf_raster_instances call (tested: 3100, four per lane of the scan,
                                      // and the refusal at 65 537 -- tests/test_gpu_limits.py)

static inline size_t rs_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct RsGeom { float x[3], y[3], i[3], pad[3]; };   // window coords (GL, y up) and 1/d of the three vertices: 48 B
struct RsModel { double m[12]; };                   // rows 0..2 of the 4x4 model-view matrix

struct RsLayout { size_t geom, bbox, cnt, off, cur, bins, total; };
static RsLayout rs_layout(int64_t n_faces, int ntiles, int64_t max_bins)
{
    RsLayout L;
    size_t o = 256;                                                       // status words {code, needed bin entries}
    L.geom = o; o += rs_align((size_t)(2 * n_faces) * sizeof(RsGeom));
    L.bbox = o; o += rs_align((size_t)(2 * n_faces) * sizeof(int4));
    L.cnt = o;  o += rs_align((size_t)ntiles * sizeof(int32_t));
    L.off = o;  o += rs_align((size_t)(ntiles + 1) * sizeof(int32_t));
    L.cur = o;  o += rs_align((size_t)ntiles * sizeof(int32_t));
    L.bins = o; o += rs_align((size_t)max_bins * sizeof(int32_t));
    L.total = o;
    return L;
}

struct RsVert { float x, y, d; };

__device__ __forceinline__ float rs_clampf(float v, float hi) { return fminf(fmaxf(v, -1.0f), hi); }

__device__ __forceinline__ void rs_emit(const RsVert& a, const RsVert& b, const RsVert& c, float p00, float p11, float hw, float hh,
                                        int W, int H, int cull, RsGeom* __restrict__ geom, int4* __restrict__ bbox, int64_t slot,
                                        int inst)
{
    const RsVert v[3] = {a, b, c};
    float x[3], y[3], iv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = ((p00 * v[k].x) / v[k].d + 1.0f) * hw;
        y[k] = ((p11 * v[k].y) / v[k].d + 1.0f) * hh;
        iv[k] = 1.0f / v[k].d;
    }
    float area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0]);
    int4 bb = make_int4(1, 1, 0, 0);                                          // empty: c0 > c1
    if (!cull && area2 < 0.0f) {                                              // back face drawn: v1 <-> v2 makes it CCW
        float t;
        t = x[1]; x[1] = x[2]; x[2] = t;
        t = y[1]; y[1] = y[2]; y[2] = t;
        t = iv[1]; iv[1] = iv[2]; iv[2] = t;
        area2 = -area2;
    }
    if (area2 > 0.0f) {
        const float xmin = fminf(fminf(x[0], x[1]), x[2]), xmax = fmaxf(fmaxf(x[0], x[1]), x[2]);
        const float ymin = fminf(fminf(y[0], y[1]), y[2]), ymax = fmaxf(fmaxf(y[0], y[1]), y[2]);
        const int c0 = max(0, (int)floorf(rs_clampf(xmin - 1.0f, (float)W)));
        const int c1 = min(W - 1, (int)floorf(rs_clampf(xmax + 1.0f, (float)W)));
        const int j0 = max(0, (int)floorf(rs_clampf(ymin - 1.0f, (float)H)));
        const int j1 = min(H - 1, (int)floorf(rs_clampf(ymax + 1.0f, (float)H)));
        if (c0 <= c1 && j0 <= j1) {
            bb = make_int4(c0, H - 1 - j1, c1, H - 1 - j0);                   // {col0, row0, col1, row1}, image rows (0 = top)
            RsGeom g;
#pragma unroll
            for (int k = 0; k < 3; ++k) { g.x[k] = x[k]; g.y[k] = y[k]; g.i[k] = iv[k]; g.pad[k] = 0.0f; }
            g.pad[0] = __int_as_float(inst);                                  // the instance that drew it (0 for a single mesh)
            geom[slot] = g;
        }
    }
    bbox[slot] = bb;
}

// the vertex of edge a (d >= zn) -> b (d < zn) on the near plane; always interpolated from the inside end, so that the two
// triangles sharing an edge get the same bits
__device__ __forceinline__ RsVert rs_clip(const RsVert& a, const RsVert& b, float zn)
{
    const float t = (a.d - zn) / (a.d - b.d);
    RsVert r;
    r.x = a.x + t * (b.x - a.x);
    r.y = a.y + t * (b.y - a.y);
    r.d = zn;
    return r;
}

// steps 1-5 of include/cppf.h for one face: `face` = its three vertex indices (local to `verts`), m = rows 0..2 of the model-view
// matrix, f = its slot (primitives 2f and 2f + 1), inst = the instance index recorded with its primitives
__device__ __forceinline__ void rs_setup_face(const double* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ face,
                                              const double* __restrict__ m, float p00, float p11, float hw, float hh, float zn, int W,
                                              int H, int cull, RsGeom* __restrict__ geom, int4* __restrict__ bbox,
                                              int32_t* __restrict__ status, int64_t f, int inst)
{
    RsVert v[3];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t vi = face[k];
        if (vi < 0 || vi >= n_verts) { bad = true; v[k] = RsVert{0.f, 0.f, 0.f}; continue; }
        const double px = verts[3 * (int64_t)vi], py = verts[3 * (int64_t)vi + 1], pz = verts[3 * (int64_t)vi + 2];
        const double cx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
        const double cy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
        const double cz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
        v[k].x = (float)cx;
        v[k].y = (float)cy;
        v[k].d = -(float)cz;
    }
    const int4 empty = make_int4(1, 1, 0, 0);
    bbox[2 * f] = empty;
    bbox[2 * f + 1] = empty;
    if (bad) { atomicCAS(status, 0, CPPF_EINVAL); return; }
    // Sutherland-Hodgman against d >= zn: <= 4 vertices, fanned from the first
    RsVert p[4];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const RsVert& a = v[k];
        const RsVert& b = v[k == 2 ? 0 : k + 1];
        const bool ia = a.d >= zn, ib = b.d >= zn;
        if (ia) p[n++] = a;
        if (ia && !ib) p[n++] = rs_clip(a, b, zn);
        if (!ia && ib) p[n++] = rs_clip(b, a, zn);
    }
    if (n >= 3) rs_emit(p[0], p[1], p[2], p00, p11, hw, hh, W, H, cull, geom, bbox, 2 * f, inst);
    if (n == 4) rs_emit(p[0], p[2], p[3], p00, p11, hw, hh, W, H, cull, geom, bbox, 2 * f + 1, inst);
}

__global__ __launch_bounds__(256) void rs_setup_kernel(const double* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                                                       int64_t n_faces, RsModel M, float p00, float p11, float hw, float hh, float zn,
                                                       int W, int H, int cull, RsGeom* __restrict__ geom, int4* __restrict__ bbox,
                                                       int32_t* __restrict__ status)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    rs_setup_face(verts, n_verts, faces + 3 * f, M.m, p00, p11, hw, hh, zn, W, H, cull, geom, bbox, status, f, 0);
}

// ---- instances: the tables cppf_raster_instances copies into its workspace (validated on the host: every inst_mesh entry names a
// mesh, both offset tables start at 0 and do not decrease)
struct RsInstTables {
    const int64_t* vert_off;      // [n_meshes + 1]
    const int64_t* face_off;      // [n_meshes + 1]
    const int32_t* inst_mesh;     // [K]
    const double* mv;             // [K, 12]
    int32_t* prefix;              // [K + 1]: instanced faces in front of instance k (rs_inst_scan_kernel)
};

// one workgroup of 1024: prefix[k] = sum over j < k of faces(inst_mesh[j]); the host has checked that the total fits 2^28
__global__ __launch_bounds__(1024) void rs_inst_scan_kernel(RsInstTables T, int K)
{
    __shared__ int part[1024];
    const int per = (K + 1023) / 1024;
    const int k0 = min(K, (int)threadIdx.x * per), k1 = min(K, k0 + per);
    int s = 0;
    for (int k = k0; k < k1; ++k) { const int m = T.inst_mesh[k]; s += (int)(T.face_off[m + 1] - T.face_off[m]); }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int k = k0; k < k1; ++k) { T.prefix[k] = run; const int m = T.inst_mesh[k]; run += (int)(T.face_off[m + 1] - T.face_off[m]); }
    if (threadIdx.x == 1023) T.prefix[K] = part[1023];
}

// one lane per instanced face q in [0, Q): its instance k is the one with prefix[k] <= q < prefix[k + 1] (every mesh has a face, so the
// prefixes increase strictly); <= 16 steps of a search in a table the whole wavefront reads together
__global__ __launch_bounds__(256) void rs_setup_inst_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            RsInstTables T, int K, int64_t Q, float p00, float p11, float hw, float hh,
                                                            float zn, int W, int H, int cull, RsGeom* __restrict__ geom,
                                                            int4* __restrict__ bbox, int32_t* __restrict__ status)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int lo = 0, hi = K;                                    // invariant: prefix[lo] <= q < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)T.prefix[mid] <= q) lo = mid; else hi = mid;
    }
    const int m = T.inst_mesh[lo];
    const int64_t v0 = T.vert_off[m], nv = T.vert_off[m + 1] - v0;
    const int64_t fl = T.face_off[m] + (q - (int64_t)T.prefix[lo]);
    rs_setup_face(verts + 3 * v0, nv, faces + 3 * fl, T.mv + 12 * (int64_t)lo, p00, p11, hw, hh, zn, W, H, cull, geom, bbox, status, q, lo);
}

__global__ __launch_bounds__(256) void rs_count_kernel(const int4* __restrict__ bbox, int64_t n_prims, int ntx, int32_t* __restrict__ cnt)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_prims; p += (int64_t)gridDim.x * 256) {
        const int4 b = bbox[p];
        if (b.x > b.z) continue;
        for (int ty = b.y / RS_TILE; ty <= b.w / RS_TILE; ++ty)
            for (int tx = b.x / RS_TILE; tx <= b.z / RS_TILE; ++tx) atomicAdd(&cnt[ty * ntx + tx], 1);
    }
}

// one workgroup of 1024: exclusive scan in int64, the capacity check, the cursors
__global__ __launch_bounds__(1024) void rs_scan_kernel(const int32_t* __restrict__ cnt, int ntiles, int64_t max_bins,
                                                       int32_t* __restrict__ off, int32_t* __restrict__ cur, int32_t* __restrict__ status)
{
    __shared__ long long part[1024];
    const int per = (ntiles + 1023) / 1024;
    const int t0 = min(ntiles, (int)threadIdx.x * per), t1 = min(ntiles, t0 + per);
    long long s = 0;
    for (int t = t0; t < t1; ++t) s += cnt[t];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const long long add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    const long long total = part[1023];
    const bool over = total > max_bins;
    if (threadIdx.x == 0) {
        status[1] = (int32_t)min(total, (long long)0x7fffffff);
        if (over && status[0] == 0) status[0] = CPPF_ECAPACITY;
    }
    if (over) return;
    long long run = part[threadIdx.x] - s;
    for (int t = t0; t < t1; ++t) { off[t] = (int32_t)run; cur[t] = (int32_t)run; run += cnt[t]; }
    if (threadIdx.x == 1023) off[ntiles] = (int32_t)total;
}

__global__ __launch_bounds__(256) void rs_scatter_kernel(const int4* __restrict__ bbox, int64_t n_prims, int ntx, int32_t* __restrict__ cur,
                                                         int32_t* __restrict__ bins, const int32_t* __restrict__ status)
{
    if (status[0] != 0) return;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_prims; p += (int64_t)gridDim.x * 256) {
        const int4 b = bbox[p];
        if (b.x > b.z) continue;
        for (int ty = b.y / RS_TILE; ty <= b.w / RS_TILE; ++ty)
            for (int tx = b.x / RS_TILE; tx <= b.z / RS_TILE; ++tx) bins[atomicAdd(&cur[ty * ntx + tx], 1)] = (int32_t)p;
    }
}

__device__ __forceinline__ float rs_edge(float ax, float ay, float bx, float by, float px, float py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
__device__ __forceinline__ bool rs_top_left(float ax, float ay, float bx, float by)
{
    const float dy = by - ay, dx = bx - ax;
    return dy < 0.0f || (dy == 0.0f && dx < 0.0f);
}
__device__ __forceinline__ bool rs_in(float w, bool tl) { return w > 0.0f || (w == 0.0f && tl); }

// LABELS: the lane also keeps the instance of its best fragment (the primitive record's spare word) and stores it to `labels`;
// on equal depth the lowest instance index wins, so the pair does not depend on the order of the bin list
template <bool LABELS>
__global__ __launch_bounds__(RS_THREADS) void rs_raster_kernel(const RsGeom* __restrict__ geom, const int4* __restrict__ bbox,
                                                               const int32_t* __restrict__ off, const int32_t* __restrict__ bins,
                                                               int ntx, int W, int H, const int32_t* __restrict__ status,
                                                               float* __restrict__ depth, int32_t* __restrict__ labels)
{
    __shared__ RsGeom sg[RS_THREADS];
    __shared__ int4 sb[RS_THREADS];
    const int tile = blockIdx.x;
    const int c = (tile % ntx) * RS_TILE + (threadIdx.x & (RS_TILE - 1));
    const int r = (tile / ntx) * RS_TILE + (threadIdx.x / RS_TILE);
    const bool own = c < W && r < H;
    if (status[0] != 0) {                                  // a bound was exceeded: NaN everywhere, never a partial image
        if (own) depth[(int64_t)r * W + c] = __int_as_float(0x7fc00000);
        if (LABELS && own) labels[(int64_t)r * W + c] = -1;
        return;
    }
    const float px = (float)c + 0.5f, py = (float)(H - 1 - r) + 0.5f;    // the pixel centre in GL window coordinates
    float best = INFINITY;
    int who = -1;
    const int b0 = off[tile], b1 = off[tile + 1];
    for (int base = b0; base < b1; base += RS_THREADS) {
        const int nb = min(RS_THREADS, b1 - base);
        __syncthreads();
        if ((int)threadIdx.x < nb) {
            const int p = bins[base + threadIdx.x];
            sg[threadIdx.x] = geom[p];
            sb[threadIdx.x] = bbox[p];
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            const int4 b = sb[j];
            if (c < b.x || c > b.z || r < b.y || r > b.w) continue;
            const RsGeom& g = sg[j];
            const float w0 = rs_edge(g.x[1], g.y[1], g.x[2], g.y[2], px, py);
            const float w1 = rs_edge(g.x[2], g.y[2], g.x[0], g.y[0], px, py);
            const float w2 = rs_edge(g.x[0], g.y[0], g.x[1], g.y[1], px, py);
            if (!rs_in(w0, rs_top_left(g.x[1], g.y[1], g.x[2], g.y[2])) || !rs_in(w1, rs_top_left(g.x[2], g.y[2], g.x[0], g.y[0])) ||
                !rs_in(w2, rs_top_left(g.x[0], g.y[0], g.x[1], g.y[1])))
                continue;
            const float d = ((w0 + w1) + w2) / ((w0 * g.i[0] + w1 * g.i[1]) + w2 * g.i[2]);
            if (LABELS) {
                const int k = __float_as_int(g.pad[0]);
                if (d < best || (d == best && k < who)) { best = d; who = k; }
            } else {
                best = d < best ? d : best;
            }
        }
    }
    if (own) depth[(int64_t)r * W + c] = best == INFINITY ? 0.0f : best;
    if (LABELS && own) labels[(int64_t)r * W + c] = best == INFINITY ? -1 : who;
}

// count, scan, scatter, raster over the primitives the set-up kernel left in the workspace; labels != NULL: the label image too.
// Returns the HIP error, or with sync the status code of the render.
static int rs_bin_and_raster(char* ws, const RsLayout& L, int64_t n_prims, int ntx, int ntiles, int W, int H, int64_t max_bin_entries,
                             float* depth, int32_t* labels, int sync, hipStream_t st)
{
    int32_t* status = reinterpret_cast<int32_t*>(ws);
    RsGeom* geom = reinterpret_cast<RsGeom*>(ws + L.geom);
    int4* bbox = reinterpret_cast<int4*>(ws + L.bbox);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
    int32_t* off = reinterpret_cast<int32_t*>(ws + L.off);
    int32_t* cur = reinterpret_cast<int32_t*>(ws + L.cur);
    int32_t* bins = reinterpret_cast<int32_t*>(ws + L.bins);
    const int64_t nblk = (n_prims + 255) / 256;
    const unsigned gp = (unsigned)(nblk < 4096 ? nblk : 4096);
    rs_count_kernel<<<gp, 256, 0, st>>>(bbox, n_prims, ntx, cnt);
    rs_scan_kernel<<<1, 1024, 0, st>>>(cnt, ntiles, max_bin_entries, off, cur, status);
    rs_scatter_kernel<<<gp, 256, 0, st>>>(bbox, n_prims, ntx, cur, bins, status);
    if (labels) rs_raster_kernel<true><<<ntiles, RS_THREADS, 0, st>>>(geom, bbox, off, bins, ntx, W, H, status, depth, labels);
    else rs_raster_kernel<false><<<ntiles, RS_THREADS, 0, st>>>(geom, bbox, off, bins, ntx, W, H, status, depth, nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (!sync) return 0;
    int32_t hs[2];
    e = hipMemcpyAsync(hs, status, sizeof(hs), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    return hs[0];
}

extern "C" size_t cppf_raster_workspace_bytes(int64_t n_faces, int W, int H, int64_t max_bin_entries)
{
    if (n_faces < 1 || W < 1 || H < 1 || W > RS_MAX_DIM || H > RS_MAX_DIM || max_bin_entries < 1 || max_bin_entries > 0x7fffffffll)
        return 0;
    const int ntiles = ((W + RS_TILE - 1) / RS_TILE) * ((H + RS_TILE - 1) / RS_TILE);
    return rs_layout(n_faces, ntiles, max_bin_entries).total;
}

extern "C" int cppf_raster_depth(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                 const double* model_view_host, double fx, double fy, int W, int H, double znear, int cull_back,
                                 float* depth, int64_t max_bin_entries, int sync, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!verts || !faces || !depth || n_verts < 1 || n_faces < 1 || n_faces > (1ll << 28) || W < 1 || H < 1 || W > RS_MAX_DIM ||
        H > RS_MAX_DIM || !(fx > 0.0) || !(fy > 0.0) || !(znear > 0.0) || max_bin_entries < 1 || max_bin_entries > 0x7fffffffll)
        return CPPF_EINVAL;
    const int ntx = (W + RS_TILE - 1) / RS_TILE, nty = (H + RS_TILE - 1) / RS_TILE, ntiles = ntx * nty;
    const RsLayout L = rs_layout(n_faces, ntiles, max_bin_entries);
    if (!workspace || workspace_bytes < L.total) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    int32_t* status = reinterpret_cast<int32_t*>(ws);
    RsGeom* geom = reinterpret_cast<RsGeom*>(ws + L.geom);
    int4* bbox = reinterpret_cast<int4*>(ws + L.bbox);
    int32_t* cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
    RsModel M;
    for (int i = 0; i < 12; ++i) M.m[i] = model_view_host ? model_view_host[i] : (i % 5 == 0 ? 1.0 : 0.0);
    const float p00 = (float)(2.0 * fx / (double)W), p11 = (float)(2.0 * fy / (double)H);
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)ntiles * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    rs_setup_kernel<<<(unsigned)((n_faces + 255) / 256), 256, 0, st>>>(verts, n_verts, faces, n_faces, M, p00, p11, hw, hh, (float)znear,
                                                                      W, H, cull_back ? 1 : 0, geom, bbox, status);
    return rs_bin_and_raster(ws, L, 2 * n_faces, ntx, ntiles, W, H, max_bin_entries, depth, nullptr, sync, st);
}

struct RsInstLayout { size_t voff, foff, imesh, mv, prefix; RsLayout L; size_t total; };
static RsInstLayout rs_inst_layout(int64_t K, int64_t Q, int64_t n_meshes, int ntiles, int64_t max_bins)
{
    RsInstLayout I;
    I.L = rs_layout(Q, ntiles, max_bins);                      // the single render's layout (status words first), the tables behind it
    size_t o = I.L.total;
    I.voff = o;   o += rs_align((size_t)(n_meshes + 1) * sizeof(int64_t));
    I.foff = o;   o += rs_align((size_t)(n_meshes + 1) * sizeof(int64_t));
    I.imesh = o;  o += rs_align((size_t)K * sizeof(int32_t));
    I.mv = o;     o += rs_align((size_t)K * 12 * sizeof(double));
    I.prefix = o; o += rs_align((size_t)(K + 1) * sizeof(int32_t));
    I.total = o;
    return I;
}

static bool rs_inst_dims_ok(int64_t K, int64_t Q, int64_t n_meshes, int W, int H, int64_t max_bins)
{
    return K >= 1 && K <= RS_MAX_INST && Q >= 1 && Q <= (1ll << 28) && n_meshes >= 1 && n_meshes <= 0x7fffffffll && W >= 1 && H >= 1 &&
           W <= RS_MAX_DIM && H <= RS_MAX_DIM && max_bins >= 1 && max_bins <= 0x7fffffffll;
}

extern "C" size_t cppf_raster_instances_workspace_bytes(int n_instances, int64_t n_inst_faces, int n_meshes, int W, int H,
                                                        int64_t max_bin_entries)
{
    if (!rs_inst_dims_ok(n_instances, n_inst_faces, n_meshes, W, H, max_bin_entries)) return 0;
    const int ntiles = ((W + RS_TILE - 1) / RS_TILE) * ((H + RS_TILE - 1) / RS_TILE);
    return rs_inst_layout(n_instances, n_inst_faces, n_meshes, ntiles, max_bin_entries).total;
}

extern "C" int cppf_raster_instances(const double* verts, const int32_t* faces, const int64_t* mesh_vert_off_host,
                                     const int64_t* mesh_face_off_host, int n_meshes, const int32_t* inst_mesh_host,
                                     const double* model_views_host, int n_instances, double fx, double fy, int W, int H, double znear,
                                     int cull_back, float* depth, int32_t* labels, int64_t max_bin_entries, int sync, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    if (!verts || !faces || !mesh_vert_off_host || !mesh_face_off_host || !inst_mesh_host || !model_views_host || !depth || !labels ||
        n_meshes < 1 || n_instances < 1 || n_instances > RS_MAX_INST || !(fx > 0.0) || !(fy > 0.0) || !(znear > 0.0))
        return CPPF_EINVAL;
    if (mesh_vert_off_host[0] != 0 || mesh_face_off_host[0] != 0) return CPPF_EINVAL;
    for (int m = 0; m < n_meshes; ++m) {                         // every mesh: 1 .. 2^28 faces, 1 .. 2^31 - 1 vertices
        const int64_t nf = mesh_face_off_host[m + 1] - mesh_face_off_host[m], nv = mesh_vert_off_host[m + 1] - mesh_vert_off_host[m];
        if (nf < 1 || nf > (1ll << 28) || nv < 1 || nv > 0x7fffffffll) return CPPF_EINVAL;
    }
    int64_t Q = 0;
    for (int k = 0; k < n_instances; ++k) {
        const int32_t m = inst_mesh_host[k];
        if (m < 0 || m >= n_meshes) return CPPF_EINVAL;
        Q += mesh_face_off_host[m + 1] - mesh_face_off_host[m];
        if (Q > (1ll << 28)) return CPPF_EINVAL;
    }
    if (!rs_inst_dims_ok(n_instances, Q, n_meshes, W, H, max_bin_entries)) return CPPF_EINVAL;
    const int ntx = (W + RS_TILE - 1) / RS_TILE, nty = (H + RS_TILE - 1) / RS_TILE, ntiles = ntx * nty;
    const RsInstLayout I = rs_inst_layout(n_instances, Q, n_meshes, ntiles, max_bin_entries);
    if (!workspace || workspace_bytes < I.total) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    int32_t* status = reinterpret_cast<int32_t*>(ws);
    RsInstTables T;
    T.vert_off = reinterpret_cast<const int64_t*>(ws + I.voff);
    T.face_off = reinterpret_cast<const int64_t*>(ws + I.foff);
    T.inst_mesh = reinterpret_cast<const int32_t*>(ws + I.imesh);
    T.mv = reinterpret_cast<const double*>(ws + I.mv);
    T.prefix = reinterpret_cast<int32_t*>(ws + I.prefix);
    const size_t ob = (size_t)(n_meshes + 1) * sizeof(int64_t);
    hipError_t e = hipMemcpyAsync(ws + I.voff, mesh_vert_off_host, ob, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + I.foff, mesh_face_off_host, ob, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + I.imesh, inst_mesh_host, (size_t)n_instances * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ws + I.mv, model_views_host, (size_t)n_instances * 12 * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(ws + I.L.cnt, 0, (size_t)ntiles * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const float p00 = (float)(2.0 * fx / (double)W), p11 = (float)(2.0 * fy / (double)H);
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    rs_inst_scan_kernel<<<1, 1024, 0, st>>>(T, n_instances);
    rs_setup_inst_kernel<<<(unsigned)((Q + 255) / 256), 256, 0, st>>>(verts, faces, T, n_instances, Q, p00, p11, hw, hh, (float)znear, W, H,
                                                                     cull_back ? 1 : 0, reinterpret_cast<RsGeom*>(ws + I.L.geom),
                                                                     reinterpret_cast<int4*>(ws + I.L.bbox), status);
    return rs_bin_and_raster(ws, I.L, 2 * Q, ntx, ntiles, W, H, max_bin_entries, depth, labels, sync, st);
}

// ----------------------------------------------------------------------------- covered pixels -> points (utils/dataset.py:203-207)
__global__ __launch_bounds__(256) void rs_valid_kernel(const float* __restrict__ depth, int64_t n, uint8_t* __restrict__ valid)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) valid[i] = depth[i] > 0.0f;
}
struct RsKinv { double k[9]; };
// backproject's arithmetic (cppf_backproject, csrc/preproc.hip), then the dataset's flips: backproject returns (-X, -Y, Z) and
// :206-207 negate x and z, so the point is (X, -Y, -Z) with (X, Y, Z) = xyz * z / xyz.z
__global__ __launch_bounds__(256) void rs_points_kernel(const float* __restrict__ depth, const int32_t* __restrict__ pix,
                                                        const int32_t* __restrict__ count, int W, RsKinv K, double* __restrict__ pts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= *count) return;
    const int p = pix[i];
    const double u = (double)(p % W), v = (double)(p / W), z = (double)depth[p];
    double xyz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xyz[c] = fma(K.k[3 * c + 1], v, K.k[3 * c] * u) + K.k[3 * c + 2];
    pts[3 * i] = xyz[0] * z / xyz[2];
    pts[3 * i + 1] = -(xyz[1] * z / xyz[2]);
    pts[3 * i + 2] = -(xyz[2] * z / xyz[2]);
}

extern "C" size_t cppf_depth_points_workspace_bytes(int H, int W)
{
    if (H < 1 || W < 1) return 0;
    const int64_t n = (int64_t)H * W;
    return rs_align((size_t)n) + cppf_compact_workspace_bytes(n);
}

extern "C" int cppf_depth_points(const float* depth, int H, int W, const double* kinv_host, double* pts, int32_t* pix, int32_t* count,
                                 void* workspace, size_t workspace_bytes, void* stream)
{
    if (H < 1 || W < 1 || (int64_t)H * W > 8192ll * 1024 || !depth || !kinv_host || !pts || !pix || !count) return CPPF_EINVAL;
    if (!workspace || workspace_bytes < cppf_depth_points_workspace_bytes(H, W)) return CPPF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W;
    uint8_t* valid = static_cast<uint8_t*>(workspace);
    char* cws = static_cast<char*>(workspace) + rs_align((size_t)n);
    const int nb = (int)((n + 255) / 256);
    rs_valid_kernel<<<nb, 256, 0, st>>>(depth, n, valid);
    const int rc = cppf_compact_mask(valid, n, pix, count, cws, cppf_compact_workspace_bytes(n), stream);
    if (rc) return rc;
    RsKinv K;
    for (int i = 0; i < 9; ++i) K.k[i] = kinv_host[i];
    rs_points_kernel<<<nb, 256, 0, st>>>(depth, pix, count, W, K, pts);
    return (int)hipGetLastError();
}
