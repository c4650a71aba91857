// k_baproblem.hip -- the set-up of Optimizer::LocalBundleAdjustment on the resident key-frame table (ref: src/Optimizer.cc:2786-2820
// lLocalMapPoints and lFixedCameras, :2888 ff. the edges).  The local points are the ordered union of
// k_localcollect.hip; these kernels add, for every local point, its observers over ALL live rows of the table in ascending
// key-frame key, and the observers that are no local key frame (the fixed ones) in the order of their first edge.
//   k_ba_rank      point j of the union leaves j + 1 in its slot's mark word (all zero between calls), as k_cull_mark leaves its id
//   k_ba_sweep     a wave per table row, twice: COUNT  cnt[j]++ for every resolving entry whose slot is marked;
//                                                FILL   the entry takes a place in the point's segment through a cursor and stores
//                                                       {rank of the row's key << 13 | feature index, row}
//   k_ba_scan      one block: cnt -> exclusive offsets, *nedges
//   k_ba_order     a wave per point: the segment in ascending sort word.  Up to 64 entries sit one per lane and every lane counts
//                  the smaller words through v_readlane; longer segments count against the segment in memory.  The ordered copy
//                  goes to a second array; a non-local row takes atomicMin(firstPos[row], place) on the way.
//   k_ba_fixed     the rows with a first place, compacted (any order), then ranked by that place: places are distinct
//   k_ba_emit      when all three counts fit the caller's room: slots, offsets, {kf, idx} edges and fixed rows to the result block
//   k_ba_unrank    the walk of k_ba_rank storing 0
// Integer atomics only, and nothing that is read back depends on which lands first: the cursor's places are re-ordered by the
// sort word (unique in a segment: one word per (row, index)), firstPos is a minimum, the compaction's order is replaced by a rank.
#include "localmap_dev.h"
#include "wave_ops.h"

#define BA_IDX_BITS 13          // KF_MAX_ROW = 1 << 13 feature indices, KF_MAX_KFS = 1 << 16 key ranks: 29 bits of sort word
#define BA_NO_POS 0xFFFFFFFFu

// hdr[0] = points (k_collect_scan), hdr[1] = edges, hdr[2] = fixed key frames
__global__ __launch_bounds__(256) void k_ba_rank(const int32_t *__restrict__ slots, const int32_t *__restrict__ hdr, int bound, int maxPoints,
                                                 uint32_t *__restrict__ marks, uint32_t store)
{
    const int n = min(hdr[0], bound);
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const int s = slots[j];
        if (s >= 0 && s < maxPoints) marks[s] = store ? (uint32_t)j + 1u : 0u;
    }
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_ba_sweep(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                  const uint32_t *__restrict__ mflags, int maxPoints, const uint32_t *__restrict__ marks,
                                                  const int32_t *__restrict__ rowRank, const int32_t *__restrict__ hdr, int bound,
                                                  uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off, uint32_t *__restrict__ cursor,
                                                  int2 *__restrict__ raw, uint32_t capRaw)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrows) return;   // wave-uniform
    const int rank = rowRank[r];
    if (rank < 0) return;     // a free row
    const uint32_t n = (uint32_t)min(hdr[0], bound);
    const int2 *row = rows + (size_t)r * stride;
    const int len = min(row[0].x, maxRow);
    for (int i = lane; i < len; i += 64) {
        const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        if (s < 0) continue;
        const uint32_t j = marks[s] - 1u;   // (unmarked: 0xFFFFFFFF)
        if (j >= n) continue;
        if (!FILL) {
            atomicAdd(cnt + j, 1u);
        } else {
            const uint32_t at = off[j] + atomicAdd(cursor + j, 1u);
            if (at < capRaw) raw[at] = make_int2((rank << BA_IDX_BITS) | i, r);
        }
    }
}

// cnt[n] -> off[n + 1] exclusive, hdr[1] = the total.  One block.
__global__ __launch_bounds__(256) void k_ba_scan(const uint32_t *__restrict__ cnt, int32_t *__restrict__ hdr, int bound,
                                                 uint32_t *__restrict__ off)
{
    __shared__ int s_wave[4];
    const int n = min(hdr[0], bound);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int running = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < n ? (int)cnt[i] : 0;
        int incl = wave_incl_scan(v);
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        const int t0 = s_wave[0], t1 = s_wave[1], t2 = s_wave[2], t3 = s_wave[3];
        incl += (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
        if (i < n) off[i] = (uint32_t)(running + incl - v);
        running += t0 + t1 + t2 + t3;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = (uint32_t)running, hdr[1] = running;
}

// raw [capRaw] {sort word, row} in cursor order -> sorted [capRaw] in ascending sort word per segment; firstPos [nrows] ~0 on entry
__global__ __launch_bounds__(256) void k_ba_order(const int2 *__restrict__ raw, const uint32_t *__restrict__ off, const int32_t *__restrict__ hdr,
                                                  int bound, uint32_t capRaw, const int32_t *__restrict__ rowLocal, int nrows,
                                                  int2 *__restrict__ sorted, uint32_t *__restrict__ firstPos)
{
    const int n = min(hdr[0], bound), lane = threadIdx.x & 63;
    for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += gridDim.x * 4) {   // wave-uniform
        const uint32_t a = off[j], b = min(off[j + 1], capRaw);
        if (a >= b) continue;
        const int len = (int)(b - a);
        if (len <= 64) {
            const int2 e = lane < len ? raw[a + lane] : make_int2(0x7FFFFFFF, -1);
            int before = 0;
            for (int k = 0; k < len; k++) before += __builtin_amdgcn_readlane(e.x, k) < e.x ? 1 : 0;
            if (lane < len) {
                const uint32_t at = a + (uint32_t)before;
                sorted[at] = e;
                if (e.y >= 0 && e.y < nrows && rowLocal[e.y] < 0) atomicMin(firstPos + e.y, at);
            }
        } else {
            for (int i = lane; i < len; i += 64) {
                const int2 e = raw[a + i];
                int before = 0;
                for (int k = 0; k < len; k++) before += raw[a + k].x < e.x ? 1 : 0;
                const uint32_t at = a + (uint32_t)before;
                sorted[at] = e;
                if (e.y >= 0 && e.y < nrows && rowLocal[e.y] < 0) atomicMin(firstPos + e.y, at);
            }
        }
    }
}

// list [nrows] = {first place, row} of the rows that have one, in any order; hdr[2] = their number
__global__ __launch_bounds__(256) void k_ba_fixed_list(const uint32_t *__restrict__ firstPos, int nrows, int32_t *__restrict__ hdr,
                                                       int2 *__restrict__ list)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t p = firstPos[r];
    if (p == BA_NO_POS) return;
    const int k = atomicAdd(hdr + 2, 1);
    if (k < nrows) list[k] = make_int2((int)p, r);
}

// fixedRank [nrows]: the place of the row among the fixed key frames (rows without a first place are never looked up)
__global__ __launch_bounds__(256) void k_ba_fixed_rank(const int2 *__restrict__ list, int nrows, const int32_t *__restrict__ hdr,
                                                       int32_t *__restrict__ fixedRank)
{
    const int nf = min(hdr[2], nrows);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < nf; k += gridDim.x * 256) {
        const int2 me = list[k];
        int before = 0;
        for (int q = 0; q < nf; q++) before += list[q].x < me.x ? 1 : 0;
        if (me.y >= 0 && me.y < nrows) fixedRank[me.y] = before;
    }
}

// res: {points, edges, fixed, 0} | slots [capP] | off [capP + 1] | fixed rows [capF] | edges [capE] {kf, idx}: the arrays only when
// every count fits
__global__ __launch_bounds__(256) void k_ba_emit(const int32_t *__restrict__ hdr, int bound, const int32_t *__restrict__ slots,
                                                 const uint32_t *__restrict__ off, const int2 *__restrict__ sorted, uint32_t capRaw,
                                                 const int2 *__restrict__ list, const int32_t *__restrict__ fixedRank,
                                                 const int32_t *__restrict__ rowLocal, int nrows, int nkf, int capP, int capE, int capF,
                                                 int32_t *__restrict__ resHdr, int32_t *__restrict__ resSlots, int32_t *__restrict__ resOff,
                                                 int32_t *__restrict__ resFixed, int2 *__restrict__ resEdges)
{
    const int np = min(hdr[0], bound), ne = (int)min((uint32_t)hdr[1], capRaw), nf = min(hdr[2], nrows);
    const int t0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    if (t0 == 0) resHdr[0] = hdr[0], resHdr[1] = hdr[1], resHdr[2] = hdr[2], resHdr[3] = 0;
    if (hdr[0] > capP || hdr[1] > capE || hdr[2] > capF || hdr[0] != np || hdr[1] != ne || hdr[2] != nf) return;
    for (int j = t0; j <= np; j += step) {
        if (j < np) resSlots[j] = slots[j];
        resOff[j] = (int32_t)off[j];
    }
    for (int k = t0; k < nf; k += step) {
        const int2 me = list[k];
        const int at = (me.y >= 0 && me.y < nrows) ? fixedRank[me.y] : -1;
        if (at >= 0 && at < nf) resFixed[at] = me.y;
    }
    for (int p = t0; p < ne; p += step) {
        const int2 e = sorted[p];
        int kf = -1;
        if (e.y >= 0 && e.y < nrows) kf = rowLocal[e.y] >= 0 ? rowLocal[e.y] : nkf + fixedRank[e.y];
        resEdges[p] = make_int2(kf, e.x & ((1 << BA_IDX_BITS) - 1));
    }
}

static int ba_grid(uint64_t items, int per)
{
    return (int)std::min<uint64_t>(std::max<uint64_t>((items + per - 1) / per, 1), 2048);
}

// After launch_collect(capOut = bound) left the union in slots and its length in hdr[0].  hdr[1], hdr[2], cnt [bound + 1] and
// cursor [bound] zero, firstPos [nrows] ~0 on entry; rowRank / rowLocal [nrows] uploaded (-1: a free row / no local key frame)
void launch_ba_problem(hipStream_t s, const void *rows, int nrows, int stride, int maxRow, const uint32_t *mflags, int maxPoints,
                       uint32_t *marks, const int32_t *rowRank, const int32_t *rowLocal, int nkf, int32_t *hdr, int bound,
                       const int32_t *slots, uint32_t *cnt, uint32_t *off, uint32_t *cursor, void *raw, void *sorted, uint32_t capRaw,
                       uint32_t *firstPos, void *list, int32_t *fixedRank, int capP, int capE, int capF, int32_t *resHdr,
                       int32_t *resSlots, int32_t *resOff, int32_t *resFixed, void *resEdges)
{
    const dim3 blk(256, 1, 1), gp(ba_grid((uint64_t)bound, 256), 1, 1), gr((nrows + 3) / 4, 1, 1);
    hipLaunchKernelGGL(k_ba_rank, gp, blk, 0, s, slots, hdr, bound, maxPoints, marks, 1u);
    hipLaunchKernelGGL(k_ba_sweep<false>, gr, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, marks, rowRank, hdr,
                       bound, cnt, off, cursor, (int2 *)raw, capRaw);
    hipLaunchKernelGGL(k_ba_scan, dim3(1, 1, 1), blk, 0, s, cnt, hdr, bound, off);
    hipLaunchKernelGGL(k_ba_sweep<true>, gr, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, marks, rowRank, hdr,
                       bound, cnt, off, cursor, (int2 *)raw, capRaw);
    hipLaunchKernelGGL(k_ba_order, dim3(ba_grid((uint64_t)bound, 4), 1, 1), blk, 0, s, (const int2 *)raw, off, hdr, bound, capRaw, rowLocal,
                       nrows, (int2 *)sorted, firstPos);
    hipLaunchKernelGGL(k_ba_fixed_list, dim3((nrows + 255) / 256, 1, 1), blk, 0, s, firstPos, nrows, hdr, (int2 *)list);
    hipLaunchKernelGGL(k_ba_fixed_rank, dim3(ba_grid((uint64_t)nrows, 256), 1, 1), blk, 0, s, (const int2 *)list, nrows, hdr, fixedRank);
    hipLaunchKernelGGL(k_ba_emit, dim3(ba_grid((uint64_t)capRaw, 256), 1, 1), blk, 0, s, hdr, bound, slots, off, (const int2 *)sorted, capRaw,
                       (const int2 *)list, fixedRank, rowLocal, nrows, nkf, capP, capE, capF, resHdr, resSlots, resOff, resFixed,
                       (int2 *)resEdges);
    hipLaunchKernelGGL(k_ba_rank, gp, blk, 0, s, slots, hdr, bound, maxPoints, marks, 0u);
}
