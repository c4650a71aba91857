// k_covis.hip -- KeyFrame::UpdateConnections' counting loop on the resident key-frame table (ref: src/KeyFrame.cc:731-765;
// DESIGN.md section 20).  w(q, j) = the number of points that are resolving entries (kf_entry_slot: live, not bad, of the entry's
// generation) of both row q and row j.  The queries go 32 to a pass: bit b of a slot's mark word (all zero between calls) says
// "query b of the pass holds this point".
//   k_covis_mark    a wave per query row: atomicOr(marks[slot], 1 << b) for every resolving entry
//   k_covis_rows    a wave per table row: the 32 counts of the row against the pass's queries, formed wave-uniformly (a ballot of
//                   bit b over the lanes and a population count: the counters live in scalar registers); every (query, row, count)
//                   with a non-zero count and row != the query's row is appended through one atomic per row
//   k_covis_clear   the walk of k_covis_mark storing 0: marks are all zero again whatever the rows kernel appended
// A point occurs at most once per row (orbhip_map_kf_put / _set refuse repeats), so a count is a number of shared points.
#include "localmap_dev.h"
#include "wave_ops.h"

#define COVIS_PASS 32

// qrows [nqp] = the table rows of the pass's queries (a row twice: two bits, the same answer twice)
template <bool CLEAR>
__device__ __forceinline__ void covis_walk(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                           const uint32_t *__restrict__ mflags, int maxPoints, const int32_t *__restrict__ qrows,
                                           int nqp, uint32_t *__restrict__ marks)
{
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nqp) return;   // wave-uniform
    const int r = qrows[b];
    if (r < 0 || r >= nrows) return;
    const int2 *row = rows + (size_t)r * stride;
    const int len = min(row[0].x, maxRow);
    for (int i = lane; i < len; i += 64) {
        const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        if (s < 0) continue;
        if (CLEAR)
            marks[s] = 0u;
        else
            atomicOr(marks + s, 1u << b);
    }
}

__global__ __launch_bounds__(256) void k_covis_mark(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                    const uint32_t *__restrict__ mflags, int maxPoints,
                                                    const int32_t *__restrict__ qrows, int nqp, uint32_t *__restrict__ marks)
{
    covis_walk<false>(rows, nrows, stride, maxRow, mflags, maxPoints, qrows, nqp, marks);
}

__global__ __launch_bounds__(256) void k_covis_clear(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                     const uint32_t *__restrict__ mflags, int maxPoints,
                                                     const int32_t *__restrict__ qrows, int nqp, uint32_t *__restrict__ marks)
{
    covis_walk<true>(rows, nrows, stride, maxRow, mflags, maxPoints, qrows, nqp, marks);
}

// *nout = number of triples appended (the caller zeroes it once per call: the passes share it), trip[k] = {query << 16 | row, count}
// for k < capOut; beyond capOut the triples are counted and not written
__global__ __launch_bounds__(256) void k_covis_rows(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                    const uint32_t *__restrict__ mflags, int maxPoints,
                                                    const uint32_t *__restrict__ marks, const int32_t *__restrict__ qrows, int nqp,
                                                    int qbase, int capOut, int32_t *__restrict__ nout, int2 *__restrict__ trip)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrows) return;   // wave-uniform
    const int2 *row = rows + (size_t)r * stride;
    const int len = min(row[0].x, maxRow);
    int cnt[COVIS_PASS];
#pragma unroll
    for (int b = 0; b < COVIS_PASS; b++) cnt[b] = 0;
    for (int base = 0; base < len; base += 64) {   // (wave-uniform trip count: every lane reaches the ballots)
        const int i = base + lane;
        uint32_t m = 0u;
        if (i < len) {
            const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
            if (s >= 0) m = marks[s];
        }
        if (__ballot(m != 0u) == 0ull) continue;
#pragma unroll
        for (int b = 0; b < COVIS_PASS; b++) cnt[b] += __popcll(__ballot((m >> b) & 1u));
    }
    int mine = 0;   // lane b < 32 takes count b
#pragma unroll
    for (int b = 0; b < COVIS_PASS; b++) mine = lane == b ? cnt[b] : mine;
    const bool put = lane < nqp && mine != 0 && qrows[lane] != r;
    const unsigned long long m = __ballot(put);
    if (m == 0ull) return;
    int at = 0;
    if (lane == 0) at = atomicAdd(nout, __popcll(m));
    at = __builtin_amdgcn_readfirstlane(at) + __popcll(m & ((1ull << lane) - 1ull));
    if (put && at < capOut) trip[at] = make_int2((int)(((uint32_t)(qbase + lane) << 16) | (uint32_t)r), mine);
}

// qrows [nq] on the device, *nout zero; the passes are enqueued back to back on s
void launch_covis(hipStream_t s, const void *rows, int nrows, int stride, int maxRow, const uint32_t *mflags, int maxPoints,
                  uint32_t *marks, const int32_t *qrows, int nq, int capOut, int32_t *nout, void *trip)
{
    if (nrows <= 0) return;
    for (int q0 = 0; q0 < nq; q0 += COVIS_PASS) {
        const int nqp = nq - q0 < COVIS_PASS ? nq - q0 : COVIS_PASS;
        const dim3 gq((nqp + 3) / 4, 1, 1), gr((nrows + 3) / 4, 1, 1), blk(256, 1, 1);
        hipLaunchKernelGGL(k_covis_mark, gq, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, qrows + q0,
                           nqp, marks);
        hipLaunchKernelGGL(k_covis_rows, gr, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, marks, qrows + q0,
                           nqp, q0, capOut, nout, (int2 *)trip);
        hipLaunchKernelGGL(k_covis_clear, gq, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, qrows + q0,
                           nqp, marks);
    }
}
