// Proposal masks -> instance clouds for gfx950 (MI355X): the dense points of up to 32 proposals of a mask-free scene, packed
// proposal by proposal in ONE pass over the dense cloud.  C ABI and the definitions: include/cppf.h ("Instance clouds of the
// proposals"); host side: cppf_amd/scene_stage.py gather_instances; restated in numpy: tests/instances_ref.py.
//   gi_count_kernel     one workgroup per chunk of CPPF_GATHER_CHUNK dense points: the membership word of every point (bit k = the
//                       sparse point that owns its voxel is in mask k) and, from wave ballots, the chunk's members per proposal
//   gi_scatter_kernel   the same chunks again: every workgroup sums the counts table itself (compact.h's self-prefix, with one
//                       counter per proposal and chunk) -- the rows before its proposal and the chunks before its own give the first
//                       output row of each of its lists -- and copies its members' 12-byte rows in dense order
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
