// Proposal masks -> instance clouds for gfx950 (MI355X): the dense points of up to 32 proposals of a mask-free scene, packed
// proposal by proposal in ONE pass over the dense cloud.  C ABI and the definitions: include/cppf.h ("Instance clouds of the
// proposals"); host side: cppf_amd/scene_stage.py gather_instances; restated in numpy: tests/instances_ref.py.
//   gi_count_kernel     one workgroup per chunk of CPPF_GATHER_CHUNK dense points: the membership word of every point (bit k = the
//                       sparse point that owns its voxel is in mask k) and, from wave ballots, the chunk's members per proposal
//   gi_scatter_kernel   the same chunks again: every workgroup sums the counts table itself (compact.h's self-prefix, with one
//                       counter per proposal and chunk) -- the rows before its proposal and the chunks before its own give the first
//                       output row of each of its lists -- and copies its members' 12-byte rows in dense order
// (cppf_gather_segments, the same packing by a per-point LABEL -- up to 1024 disjoint segments in one call -- is the second half of
// this file.)
// Both are bound by memory and by the byte gathers into the masks (n_props per point, neighbours in the dense cloud share their
// owner).  No atomics: a count is a population count of a ballot, a position is a prefix of counts, the same words on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cppf.h"

#define GI_MAX_K 32                      // one bit per proposal in a 32-bit word (scene_multi.hip: BVM_MAX_CENTERS)
#define GI_CHUNK CPPF_GATHER_CHUNK
#define GI_WAVES (GI_CHUNK / 64)

// member[i] and counts[k][chunk]; a chunk that holds an owner >= n_sparse writes -1 into all of its counts instead (and 0 into those
// points' words): gi_scatter_kernel reads every count, so every workgroup of it learns of the refusal
__global__ __launch_bounds__(GI_CHUNK) void gi_count_kernel(const int32_t* __restrict__ owner, const uint8_t* __restrict__ masks,
                                                            int n_props, int64_t n_sparse, int64_t n_dense,
                                                            uint32_t* __restrict__ member, int32_t* __restrict__ counts, int64_t n_chunks)
{
    __shared__ int wsum[GI_WAVES][GI_MAX_K];
    __shared__ int wbad[GI_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * GI_CHUNK + threadIdx.x;
    uint32_t word = 0;
    bool bad = false;
    if (i < n_dense) {
        const int32_t o = owner[i];
        bad = o >= n_sparse;
        if (o >= 0 && !bad)
            for (int k = 0; k < n_props; ++k) word |= (masks[(int64_t)k * n_sparse + o] ? 1u : 0u) << k;
        member[i] = word;
    }
    int mine = 0;
    for (int k = 0; k < n_props; ++k) {
        const int c = __popcll(__ballot((word >> k) & 1u));
        if (lane == k) mine = c;
    }
    if (lane < n_props) wsum[w][lane] = mine;
    const unsigned long long anybad = __ballot(bad);
    if (lane == 0) wbad[w] = anybad != 0ull;
    __syncthreads();
    if ((int)threadIdx.x < n_props) {
        int s = 0, b = 0;
        for (int j = 0; j < GI_WAVES; ++j) { s += wsum[j][threadIdx.x]; b |= wbad[j]; }
        counts[(int64_t)threadIdx.x * n_chunks + blockIdx.x] = b ? -1 : s;
    }
}

// rows offsets[k] + (members of proposal k in the chunks before this one) + (rank within the chunk) of pts / nrm / src <- the chunk's
// members of proposal k; rows >= capacity are dropped.  Workgroup 0 writes offsets.  A negative count anywhere: nothing is copied
// and offsets = {0, ..., 0, -1}.  Launch: max(n_chunks, 1) workgroups.
__global__ __launch_bounds__(GI_CHUNK) void gi_scatter_kernel(const float* __restrict__ hi, const float* __restrict__ hi_nrm,
                                                              const uint32_t* __restrict__ member, int n_props, int64_t n_dense,
                                                              const int32_t* __restrict__ counts, int64_t n_chunks, int64_t capacity,
                                                              int32_t* __restrict__ offsets, float* __restrict__ pts,
                                                              float* __restrict__ nrm, int32_t* __restrict__ src)
{
    __shared__ int row_total[GI_MAX_K], row_before[GI_MAX_K], row_base[GI_MAX_K];
    __shared__ int wsum[GI_WAVES][GI_MAX_K], wpre[GI_WAVES][GI_MAX_K];
    __shared__ int wbad[GI_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the table, once: wave w sums rows w and w + GI_WAVES -- the whole row and the part in front of this chunk
    int neg = 0;
    for (int k = w; k < n_props; k += GI_WAVES) {
        const int32_t* row = counts + (int64_t)k * n_chunks;
        int tot = 0, before = 0;
        for (int64_t c = lane; c < n_chunks; c += 64) {
            const int v = row[c];
            neg |= v < 0;
            tot += v;
            before += c < (int64_t)blockIdx.x ? v : 0;
        }
        for (int off = 32; off > 0; off >>= 1) {
            tot += __shfl_xor(tot, off, 64);
            before += __shfl_xor(before, off, 64);
        }
        if (lane == 0) { row_total[k] = tot; row_before[k] = before; }
    }
    const unsigned long long anyneg = __ballot(neg);
    if (lane == 0) wbad[w] = anyneg != 0ull;
    __syncthreads();
    int bad = 0;
    for (int j = 0; j < GI_WAVES; ++j) bad |= wbad[j];
    if (bad) {
        if (blockIdx.x == 0 && (int)threadIdx.x <= n_props) offsets[threadIdx.x] = (int)threadIdx.x == n_props ? -1 : 0;
        return;
    }
    if ((int)threadIdx.x <= n_props) {
        int base = 0;
        for (int k = 0; k < (int)threadIdx.x; ++k) base += row_total[k];
        if (blockIdx.x == 0) offsets[threadIdx.x] = base;
        if ((int)threadIdx.x < n_props) row_base[threadIdx.x] = base + row_before[threadIdx.x];
    }
    // this chunk's members: per proposal the waves' counts, then their exclusive prefix over the waves
    const int64_t i = (int64_t)blockIdx.x * GI_CHUNK + threadIdx.x;
    const uint32_t word = i < n_dense ? member[i] : 0u;
    int mine = 0;
    for (int k = 0; k < n_props; ++k) {
        const int c = __popcll(__ballot((word >> k) & 1u));
        if (lane == k) mine = c;
    }
    if (lane < n_props) wsum[w][lane] = mine;
    __syncthreads();
    if ((int)threadIdx.x < n_props) {
        int acc = 0;
        for (int j = 0; j < GI_WAVES; ++j) { wpre[j][threadIdx.x] = acc; acc += wsum[j][threadIdx.x]; }
    }
    __syncthreads();
    float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
    if (word) {
        for (int e = 0; e < 3; ++e) { p[e] = hi[3 * i + e]; q[e] = hi_nrm[3 * i + e]; }
    }
    for (int k = 0; k < n_props; ++k) {
        const bool f = (word >> k) & 1u;
        const unsigned long long b = __ballot(f);
        if (b == 0ull) continue;
        if (f) {
            const int64_t pos = (int64_t)row_base[k] + wpre[w][k] + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < capacity) {
                for (int e = 0; e < 3; ++e) { pts[3 * pos + e] = p[e]; nrm[3 * pos + e] = q[e]; }
                src[pos] = (int32_t)i;
            }
        }
    }
}

extern "C" int cppf_gather_instances(const float* hi, const float* hi_nrm, const int32_t* owner, const uint8_t* masks, int n_props,
                                     int64_t n_sparse, int64_t n_dense, int64_t capacity, uint32_t* member, int32_t* offsets,
                                     float* pts, float* nrm, int32_t* src, int32_t* chunk_counts, void* stream)
{
    if (n_props < 1 || n_props > GI_MAX_K || n_sparse < 0 || n_dense < 0 || capacity < 0) return CPPF_EINVAL;
    if (n_dense > INT32_MAX || n_dense * n_props > INT32_MAX || n_sparse > INT32_MAX) return CPPF_EINVAL;     // offsets, src and owner are int32
    if (!offsets || (capacity > 0 && (!pts || !nrm || !src))) return CPPF_EINVAL;
    if (n_dense > 0 && (!hi || !hi_nrm || !owner || !member || !chunk_counts || (n_sparse > 0 && !masks))) return CPPF_EINVAL;
    const int64_t nc = (n_dense + GI_CHUNK - 1) / GI_CHUNK;
    if (nc > CPPF_GATHER_MAX_CHUNKS) return CPPF_EUNSUPPORTED;       // every scatter workgroup sums the whole counts table
    hipStream_t st = (hipStream_t)stream;
    if (nc > 0)
        hipLaunchKernelGGL(gi_count_kernel, dim3((unsigned)nc), dim3(GI_CHUNK), 0, st, owner, masks, n_props, n_sparse, n_dense, member,
                           chunk_counts, nc);
    hipLaunchKernelGGL(gi_scatter_kernel, dim3((unsigned)(nc > 0 ? nc : 1)), dim3(GI_CHUNK), 0, st, hi, hi_nrm, member, n_props, n_dense,
                       chunk_counts, nc, capacity, offsets, pts, nrm, src);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Segment labels -> segment clouds: cppf_gather_segments, a stable partition of the dense cloud by label (include/cppf.h "Segment
// clouds"; host side: cppf_amd/segments.py segment_clouds; restated in numpy: tests/gather_segments_ref.py).
//   gs_count_kernel     one workgroup per chunk of CPPF_GATHER_CHUNK points: the chunk's points per label (gs_rank's per-wave counts,
//                       summed over the waves) -> counts[chunk][label]; workgroup 0 also fills bounds with the empty values
//   gs_scan_kernel      64 labels per workgroup, lane = label, wave = a sixteenth of the chunks: counts[.][label] <- its exclusive
//                       prefix over the chunks, in place; the label's total -> offsets[label + 1]
//   gs_offsets_kernel   one workgroup: offsets <- the prefix of the totals
//   gs_scatter_kernel   the chunks again: row = offsets[label] + counts[chunk][label] + (the label's points in the waves before this
//                       one) + (its points in the lanes below this one); the bounds by integer min / max on the floats' bits
// The table is chunk-major, so that a wave reads and writes 64 neighbouring labels of one chunk at once.  The only atomics are integer
// min / max (in LDS, then one per touched label and workgroup in memory): order does not matter to them, the same words on every run.
#define GS_MAX_S CPPF_GATHER_SEGMENTS_MAX
static_assert(GS_MAX_S == GI_CHUNK, "thread s of a chunk's workgroup serves label s");
static_assert(GS_MAX_S == CPPF_SEGMENTS_MAX, "a label of cppf_depth_segments is a segment here");

// The stable rank of a lane among the lanes of its wave with the same label (ok = false: no label), and by the way cnt[label] <- the
// number of such lanes, for every label in the wave: one trip per distinct label -- the first lane still waiting names the label, a
// ballot finds its lanes.  Labels of neighbouring pixels agree, so a wave mostly takes one or two trips (64 at the worst).
__device__ __forceinline__ int gs_rank(int label, bool ok, int lane, uint16_t* __restrict__ cnt)
{
    int rank = 0;
    bool waiting = ok;
    for (;;) {
        const unsigned long long todo = __ballot(waiting);
        if (todo == 0ull) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int l = __shfl(label, leader, 64);
        const bool mine = waiting && label == l;
        const unsigned long long b = __ballot(mine);
        if (mine) {
            rank = __popcll(b & ((1ull << lane) - 1ull));
            waiting = false;
            if (lane == leader) cnt[l] = (uint16_t)__popcll(b);
        }
    }
    return rank;
}

__device__ __forceinline__ void gs_zero(uint16_t (*wcnt)[GS_MAX_S])
{
    uint32_t* z = (uint32_t*)&wcnt[0][0];
    for (int j = threadIdx.x; j < GI_WAVES * GS_MAX_S / 2; j += GI_CHUNK) z[j] = 0u;
}

// min / max in the order of the sign-magnitude key (-0.0 below +0.0) by integer atomics on the floats' own bits: among non-negative
// floats the order is the signed integers', among negative ones the reverse of the unsigned integers', and every negative float
// is a larger unsigned and a smaller signed integer than every non-negative one.  v: the bits of a value that is not NaN.
template <typename T> __device__ __forceinline__ void gs_min(T* p, uint32_t v)
{
    if (v >> 31) atomicMax((unsigned int*)p, v); else atomicMin((int*)p, (int)v);
}
template <typename T> __device__ __forceinline__ void gs_max(T* p, uint32_t v)
{
    if (v >> 31) atomicMin((unsigned int*)p, v); else atomicMax((int*)p, (int)v);
}
#define GS_PINF 0x7f800000u
#define GS_NINF 0xff800000u

__global__ __launch_bounds__(GI_CHUNK) void gs_count_kernel(const int32_t* __restrict__ labels, int n_seg, int64_t n_dense,
                                                            int32_t* __restrict__ counts, uint32_t* __restrict__ bounds)
{
    __shared__ uint16_t wcnt[GI_WAVES][GS_MAX_S];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    gs_zero(wcnt);
    if (bounds && blockIdx.x == 0 && (int)threadIdx.x < n_seg)
        for (int e = 0; e < 6; ++e) bounds[6 * threadIdx.x + e] = e < 3 ? GS_PINF : GS_NINF;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * GI_CHUNK + threadIdx.x;
    const int32_t l = i < n_dense ? labels[i] : -1;
    gs_rank(l, (uint32_t)l < (uint32_t)n_seg, lane, wcnt[w]);
    __syncthreads();
    if ((int)threadIdx.x < n_seg) {
        int s = 0;
        for (int j = 0; j < GI_WAVES; ++j) s += wcnt[j][threadIdx.x];
        counts[(int64_t)blockIdx.x * n_seg + threadIdx.x] = s;
    }
}

// launch: ceil(n_seg / 64) workgroups of GI_CHUNK threads
__global__ __launch_bounds__(GI_CHUNK) void gs_scan_kernel(int32_t* __restrict__ counts, int n_seg, int64_t n_chunks,
                                                           int32_t* __restrict__ offsets)
{
    __shared__ int part[GI_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane;
    const int64_t per = (n_chunks + GI_WAVES - 1) / GI_WAVES;
    const int64_t c0 = w * per < n_chunks ? w * per : n_chunks, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
    int sum = 0;
    if (s < n_seg)
        for (int64_t c = c0; c < c1; ++c) sum += counts[c * n_seg + s];
    part[w][lane] = sum;
    __syncthreads();
    if (s >= n_seg) return;
    int run = 0, total = 0;
    for (int j = 0; j < GI_WAVES; ++j) { run += j < w ? part[j][lane] : 0; total += part[j][lane]; }
    if (w == 0) offsets[s + 1] = total;
    for (int64_t c = c0; c < c1; ++c) {
        const int v = counts[c * n_seg + s];
        counts[c * n_seg + s] = run;
        run += v;
    }
}

// offsets[1 + s] holds label s's total; offsets <- {0, the inclusive prefix of the totals}.  One workgroup of GI_CHUNK threads.
__global__ __launch_bounds__(GI_CHUNK) void gs_offsets_kernel(int32_t* __restrict__ offsets, int n_seg)
{
    __shared__ int wtot[GI_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int v = (int)threadIdx.x < n_seg ? offsets[threadIdx.x + 1] : 0;
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    for (int j = 0; j < w; ++j) v += wtot[j];
    if ((int)threadIdx.x < n_seg) offsets[threadIdx.x + 1] = v;
    if (threadIdx.x == 0) offsets[0] = 0;
}

__global__ __launch_bounds__(GI_CHUNK) void gs_scatter_kernel(const float* __restrict__ hi, const float* __restrict__ hi_nrm,
                                                              const int32_t* __restrict__ labels, int n_seg, int64_t n_dense,
                                                              const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                                                              int64_t capacity, float* __restrict__ pts, float* __restrict__ nrm,
                                                              int32_t* __restrict__ src, uint32_t* __restrict__ bounds)
{
    __shared__ uint16_t wcnt[GI_WAVES][GS_MAX_S];
    __shared__ int row_base[GS_MAX_S];
    __shared__ uint32_t box[6][GS_MAX_S];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    gs_zero(wcnt);
    if ((int)threadIdx.x < n_seg) {
        row_base[threadIdx.x] = offsets[threadIdx.x] + counts[(int64_t)blockIdx.x * n_seg + threadIdx.x];
        if (bounds)
            for (int e = 0; e < 6; ++e) box[e][threadIdx.x] = e < 3 ? GS_PINF : GS_NINF;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * GI_CHUNK + threadIdx.x;
    const int32_t l = i < n_dense ? labels[i] : -1;
    const bool ok = (uint32_t)l < (uint32_t)n_seg;
    const int rank = gs_rank(l, ok, lane, wcnt[w]);
    __syncthreads();
    int here = 0;                                                             // label threadIdx.x's points in this chunk
    if ((int)threadIdx.x < n_seg)
        for (int j = 0; j < GI_WAVES; ++j) { const int c = wcnt[j][threadIdx.x]; wcnt[j][threadIdx.x] = (uint16_t)here; here += c; }
    __syncthreads();
    if (ok) {
        float p[3], q[3];
        for (int e = 0; e < 3; ++e) { p[e] = hi[3 * i + e]; q[e] = hi_nrm[3 * i + e]; }
        const int64_t pos = (int64_t)row_base[l] + wcnt[w][l] + rank;
        if (pos < capacity) {
            for (int e = 0; e < 3; ++e) { pts[3 * pos + e] = p[e]; nrm[3 * pos + e] = q[e]; }
            src[pos] = (int32_t)i;
        }
        if (bounds) {
            const uint32_t b[3] = {__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2])};
            if ((b[0] & GS_PINF) != GS_PINF && (b[1] & GS_PINF) != GS_PINF && (b[2] & GS_PINF) != GS_PINF)      // all three finite
                for (int e = 0; e < 3; ++e) { gs_min(&box[e][l], b[e]); gs_max(&box[3 + e][l], b[e]); }
        }
    }
    if (!bounds) return;
    __syncthreads();
    if (here > 0)
        for (int e = 0; e < 3; ++e) {
            gs_min(&bounds[6 * threadIdx.x + e], box[e][threadIdx.x]);
            gs_max(&bounds[6 * threadIdx.x + 3 + e], box[3 + e][threadIdx.x]);
        }
}

// n_dense = 0: offsets all zero, bounds empty.  One workgroup of GI_CHUNK threads.
__global__ __launch_bounds__(GI_CHUNK) void gs_empty_kernel(int32_t* __restrict__ offsets, uint32_t* __restrict__ bounds, int n_seg)
{
    if ((int)threadIdx.x <= n_seg) offsets[threadIdx.x] = 0;
    if ((int)threadIdx.x == GI_CHUNK - 1) offsets[n_seg] = 0;                 // (n_seg = 1024: one entry more than threads)
    if (bounds && (int)threadIdx.x < n_seg)
        for (int e = 0; e < 6; ++e) bounds[6 * threadIdx.x + e] = e < 3 ? GS_PINF : GS_NINF;
}

extern "C" int cppf_gather_segments(const float* hi, const float* hi_nrm, const int32_t* labels, int n_segments, int64_t n_dense,
                                    int64_t capacity, int32_t* offsets, float* pts, float* nrm, int32_t* src, float* bounds,
                                    int32_t* chunk_counts, void* stream)
{
    if (n_segments < 1 || n_segments > GS_MAX_S || n_dense < 0 || capacity < 0) return CPPF_EINVAL;
    if (n_dense > INT32_MAX) return CPPF_EINVAL;                              // offsets and src are int32
    if (!offsets || (capacity > 0 && (!pts || !nrm || !src))) return CPPF_EINVAL;
    if (n_dense > 0 && (!hi || !hi_nrm || !labels || !chunk_counts)) return CPPF_EINVAL;
    const int64_t nc = (n_dense + GI_CHUNK - 1) / GI_CHUNK;
    if (nc > CPPF_GATHER_MAX_CHUNKS) return CPPF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* box = (uint32_t*)bounds;
    if (nc == 0) {
        hipLaunchKernelGGL(gs_empty_kernel, dim3(1), dim3(GI_CHUNK), 0, st, offsets, box, n_segments);
    } else {
        hipLaunchKernelGGL(gs_count_kernel, dim3((unsigned)nc), dim3(GI_CHUNK), 0, st, labels, n_segments, n_dense, chunk_counts, box);
        hipLaunchKernelGGL(gs_scan_kernel, dim3((unsigned)((n_segments + 63) / 64)), dim3(GI_CHUNK), 0, st, chunk_counts, n_segments, nc,
                           offsets);
        hipLaunchKernelGGL(gs_offsets_kernel, dim3(1), dim3(GI_CHUNK), 0, st, offsets, n_segments);
        hipLaunchKernelGGL(gs_scatter_kernel, dim3((unsigned)nc), dim3(GI_CHUNK), 0, st, hi, hi_nrm, labels, n_segments, n_dense,
                           chunk_counts, offsets, capacity, pts, nrm, src, box);
    }
    if (hipError_t e = hipGetLastError()) return (int)e;
    return 0;
}
