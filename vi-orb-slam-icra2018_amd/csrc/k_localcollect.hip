// k_localcollect.hip -- Tracking::UpdateLocalMap on the resident store (ref: src/Tracking.cc:2377-2400 UpdateLocalPoints,
// :2411-2429 the vote of UpdateLocalKeyFrames).
// The key-frame table: one fixed-stride row of int2 per key frame, entry 0 = {used length, 0}, entry 1 + i = {slot, generation}
// of KeyFrame::mvpMapPoints[i] ({-1, 0}: no point).  An entry names a point only while the slot's flag word (k_localmap.hip)
// is live and carries the entry's generation in its bits 8..31: an erased or re-used slot never resolves.
//   k_mark_add / k_mark_clear   scatter +1 / 0 into the per-slot mark words: the frame's points with their multiplicity (vote),
//                               the frame's own matches (the skip bytes of the fused call); cleared by the same scatter
//   k_kf_set                    single row entries
//   k_vote_rows                 a wave per row: the sum of the marks of its live, non-bad entries; rows with a non-zero sum are
//                               appended to the output (the host orders them by key)
//   k_collect_first             a lane per candidate position p = row offset in the call + feature index: atomicMin(first[slot], p)
//   k_collect_count / _scan / _write   order-preserving compaction of the candidates with first[slot] == p: block counts, one
//                               block's scan over them, scatter.  The survivors put first[slot] back to ~0, so no pass over the
//                               store is ever needed.
#include "localmap_dev.h"
#include "wave_ops.h"

#define COLLECT_BLOCK 256
#define NO_FIRST 0xFFFFFFFFu

__global__ __launch_bounds__(256) void k_mark_add(const int32_t *__restrict__ slots, int n, int maxPoints, uint32_t *__restrict__ marks)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s >= 0 && s < maxPoints) atomicAdd(marks + s, 1u);
}

__global__ __launch_bounds__(256) void k_mark_clear(const int32_t *__restrict__ slots, int n, int maxPoints, uint32_t *__restrict__ marks)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s >= 0 && s < maxPoints) marks[s] = 0u;
}

__global__ __launch_bounds__(256) void k_kf_set(const int64_t *__restrict__ at, const int2 *__restrict__ val, int m, int64_t total,
                                                int2 *__restrict__ rows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t a = at[i];
    if (a >= 0 && a < total) rows[a] = val[i];
}

// *nout = number of rows appended (zero on entry), pairs[2k], pairs[2k + 1] = row, count
__global__ __launch_bounds__(256) void k_vote_rows(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                   const uint32_t *__restrict__ mflags, int maxPoints,
                                                   const uint32_t *__restrict__ marks, int capOut, int32_t *__restrict__ nout,
                                                   int32_t *__restrict__ pairs)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrows) return;   // wave-uniform
    const int2 *row = rows + (size_t)r * stride;
    const int len = min(row[0].x, maxRow);
    int sum = 0;
    for (int i = lane; i < len; i += 64) {
        const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        if (s >= 0) sum += (int)marks[s];
    }
    sum = wave_sum(sum);
    if (lane == 0 && sum != 0) {
        const int k = atomicAdd(nout, 1);
        if (k < capOut) pairs[2 * k] = r, pairs[2 * k + 1] = sum;
    }
}

// cand[p] = the slot of candidate p or -1; first[slot] = the smallest p that names it
__global__ __launch_bounds__(COLLECT_BLOCK) void k_collect_first(const int2 *__restrict__ rows, int nrows, int stride,
                                                                 const int32_t *__restrict__ rowIdx,
                                                                 const uint32_t *__restrict__ off, int nkf,
                                                                 const uint32_t *__restrict__ mflags, int maxPoints,
                                                                 int32_t *__restrict__ cand, uint32_t *__restrict__ first)
{
    const uint32_t p = blockIdx.x * COLLECT_BLOCK + threadIdx.x;
    if (p >= off[nkf]) return;
    int lo = 0, hi = nkf;   // the row k with off[k] <= p < off[k + 1] (rows of length 0 are never chosen)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    const int r = rowIdx[lo];
    int s = -1;
    if (r >= 0 && r < nrows) s = kf_entry_slot(rows[(size_t)r * stride + 1 + (p - off[lo])], mflags, maxPoints);
    cand[p] = s;
    if (s >= 0) atomicMin(first + s, p);
}

// the number of survivors of this block in front of this thread's candidate; *total = the block's (every thread of the block calls it)
__device__ __forceinline__ int collect_block_rank(bool surv, int *total)
{
    __shared__ int s_wave[COLLECT_BLOCK / 64];
    const unsigned long long m = __ballot(surv);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < COLLECT_BLOCK / 64; k++) {
        before += k < w ? s_wave[k] : 0;
        all += s_wave[k];
    }
    *total = all;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(COLLECT_BLOCK) void k_collect_count(const int32_t *__restrict__ cand, uint32_t P,
                                                                 const uint32_t *__restrict__ first, int32_t *__restrict__ blockCnt)
{
    const uint32_t p = blockIdx.x * COLLECT_BLOCK + threadIdx.x;
    const int s = p < P ? cand[p] : -1;
    int total;
    (void)collect_block_rank(s >= 0 && first[s] == p, &total);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = total;
}

// blockCnt[nb] -> exclusive prefix sums in place, *nlocal = the total.  One block.
__global__ __launch_bounds__(256) void k_collect_scan(int32_t *__restrict__ blockCnt, int nb, int32_t *__restrict__ nlocal)
{
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int running = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? blockCnt[i] : 0;
        int incl = wave_incl_scan(v);
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        const int t0 = s_wave[0], t1 = s_wave[1], t2 = s_wave[2], t3 = s_wave[3];
        incl += (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
        if (i < nb) blockCnt[i] = running + incl - v;
        running += t0 + t1 + t2 + t3;
        __syncthreads();
    }
    if (threadIdx.x == 0) *nlocal = running;
}

// survivors in order -> slots[capOut] (and skip[capOut] = the slot is marked, when asked for); first[] as it was before the call
__global__ __launch_bounds__(COLLECT_BLOCK) void k_collect_write(const int32_t *__restrict__ cand, uint32_t P,
                                                                 uint32_t *__restrict__ first, const int32_t *__restrict__ blockOff,
                                                                 const uint32_t *__restrict__ marks, int capOut,
                                                                 int32_t *__restrict__ slots, uint8_t *__restrict__ skip)
{
    const uint32_t p = blockIdx.x * COLLECT_BLOCK + threadIdx.x;
    const int s = p < P ? cand[p] : -1;
    const bool surv = s >= 0 && first[s] == p;
    int total;
    const int k = blockOff[blockIdx.x] + collect_block_rank(surv, &total);
    if (!surv) return;
    first[s] = NO_FIRST;   // (a later candidate of the same slot compares against its own p: neither value is equal to it)
    if (k >= capOut) return;
    slots[k] = s;
    if (skip) skip[k] = marks[s] != 0u ? 1 : 0;
}

void launch_mark_add(hipStream_t s, const int32_t *slots, int n, int maxPoints, uint32_t *marks)
{
    if (n > 0) hipLaunchKernelGGL(k_mark_add, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slots, n, maxPoints, marks);
}

void launch_mark_clear(hipStream_t s, const int32_t *slots, int n, int maxPoints, uint32_t *marks)
{
    if (n > 0) hipLaunchKernelGGL(k_mark_clear, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slots, n, maxPoints, marks);
}

void launch_kf_set(hipStream_t s, const int64_t *at, const void *val, int m, int64_t total, void *rows)
{
    if (m > 0) hipLaunchKernelGGL(k_kf_set, dim3((m + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, at, (const int2 *)val, m, total, (int2 *)rows);
}

void launch_vote_rows(hipStream_t s, const void *rows, int nrows, int stride, int maxRow, const uint32_t *mflags, int maxPoints,
                      const uint32_t *marks, int capOut, int32_t *nout, int32_t *pairs)
{
    if (nrows > 0)
        hipLaunchKernelGGL(k_vote_rows, dim3((nrows + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, (const int2 *)rows, nrows, stride, maxRow,
                           mflags, maxPoints, marks, capOut, nout, pairs);
}

int collect_blocks(uint32_t P) { return (int)((P + COLLECT_BLOCK - 1) / COLLECT_BLOCK); }

// P = off[nkf] > 0 candidates; cand[P], blockCnt[collect_blocks(P)] scratch; *nlocal is written, slots[capOut] (skip[capOut])
void launch_collect(hipStream_t s, const void *rows, int nrows, int stride, const int32_t *rowIdx, const uint32_t *off, int nkf,
                    uint32_t P, const uint32_t *mflags, int maxPoints, const uint32_t *marks, uint32_t *first, int32_t *cand,
                    int32_t *blockCnt, int capOut, int32_t *slots, uint8_t *skip, int32_t *nlocal)
{
    const int nb = collect_blocks(P);
    hipLaunchKernelGGL(k_collect_first, dim3(nb, 1, 1), dim3(COLLECT_BLOCK, 1, 1), 0, s, (const int2 *)rows, nrows, stride, rowIdx, off,
                       nkf, mflags, maxPoints, cand, first);
    hipLaunchKernelGGL(k_collect_count, dim3(nb, 1, 1), dim3(COLLECT_BLOCK, 1, 1), 0, s, cand, P, first, blockCnt);
    hipLaunchKernelGGL(k_collect_scan, dim3(1, 1, 1), dim3(256, 1, 1), 0, s, blockCnt, nb, nlocal);
    hipLaunchKernelGGL(k_collect_write, dim3(nb, 1, 1), dim3(COLLECT_BLOCK, 1, 1), 0, s, cand, P, first, blockCnt, marks, capOut, slots,
                       skip);
}
