// k_cull.hip -- the counting loop of LocalMapping::KeyFrameCulling / KeyFrameCullingForMonoVI on the resident key-frame table
// (ref: src/LocalMapping.cc:1533-1581, :2705-2753).  For every candidate key frame: how many of its points
// count (n_mps) and how many of those are seen by at least th_obs other key frames at the same or a finer scale (n_redundant).
// A row entry resolves as everywhere (kf_entry_slot: live, not bad, of the entry's generation); its level byte (levels
// [maxKfs][maxRow], parallel to the rows) holds the feature's octave in bits 0..3, "counts twice in nObs" in bit 6, "far" in bit 7.
//   k_cull_mark    a wave per candidate row: every resolving entry claims its slot's mark word (all zero between calls); the
//                  claimer takes a compact id from one counter and leaves id + 1 in the word.  One id per point of the call.
//   k_cull_tally   a wave per table row, one sweep for all candidates: tally[id][octave]++ and tally[id][16] += 1 + stereo for
//                  every resolving entry whose slot is marked.  tally[id][0..15] = observers by octave, [16] = Observations().
//   k_cull_count   a wave per candidate: others = the prefix of the point's octave counts up to min(l + 1, 15), minus the
//                  candidate's own entry (octave l lies inside the prefix); two wave sums; the entry states
//   k_cull_clear   the walk of k_cull_mark storing 0: the marks are zero again whatever happened in between
// Nothing depends on which atomic lands first: the ids differ between runs, the sums do not.
#include "localmap_dev.h"
#include "wave_ops.h"

#define CULL_COLS 17
#define CULL_CLAIMED 0xFFFFFFFFu   // between the claim and the id (never read as an id: the kernel ends in between)

// cand [K] = {table row, the row's length as the host knows it}
__global__ __launch_bounds__(256) void k_cull_mark(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                   const uint32_t *__restrict__ mflags, int maxPoints, const int2 *__restrict__ cand,
                                                   int K, uint32_t *__restrict__ marks, uint32_t *__restrict__ nids)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;   // wave-uniform
    const int2 cd = cand[k];
    if (cd.x < 0 || cd.x >= nrows) return;
    const int2 *row = rows + (size_t)cd.x * stride;
    const int len = min(min(row[0].x, cd.y), maxRow);
    for (int base = 0; base < len; base += 64) {   // (wave-uniform trip count: every lane reaches the ballot)
        const int i = base + lane;
        int s = -1;
        if (i < len) s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        const bool mine = s >= 0 && atomicCAS(marks + s, 0u, CULL_CLAIMED) == 0u;
        const unsigned long long m = __ballot(mine);
        if (m == 0ull) continue;
        uint32_t at = 0u;
        if (lane == 0) at = atomicAdd(nids, (uint32_t)__popcll(m));
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (mine) marks[s] = at + 1u;
    }
}

__global__ __launch_bounds__(256) void k_cull_clear(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                    const uint32_t *__restrict__ mflags, int maxPoints, const int2 *__restrict__ cand,
                                                    int K, uint32_t *__restrict__ marks)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;   // wave-uniform
    const int2 cd = cand[k];
    if (cd.x < 0 || cd.x >= nrows) return;
    const int2 *row = rows + (size_t)cd.x * stride;
    const int len = min(min(row[0].x, cd.y), maxRow);
    for (int i = lane; i < len; i += 64) {
        const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        if (s >= 0) marks[s] = 0u;
    }
}

// tally [bound][17], zero on entry
__global__ __launch_bounds__(256) void k_cull_tally(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                    const uint8_t *__restrict__ levels, const uint32_t *__restrict__ mflags,
                                                    int maxPoints, const uint32_t *__restrict__ marks, uint32_t bound,
                                                    uint32_t *__restrict__ tally)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= nrows) return;   // wave-uniform
    const int2 *row = rows + (size_t)r * stride;
    const uint8_t *lv = levels + (size_t)r * maxRow;
    const int len = min(row[0].x, maxRow);
    for (int i = lane; i < len; i += 64) {
        const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
        if (s < 0) continue;
        const uint32_t id = marks[s] - 1u;   // (unmarked: 0xFFFFFFFF)
        if (id >= bound) continue;
        const uint32_t b = lv[i];
        uint32_t *t = tally + (size_t)id * CULL_COLS;
        atomicAdd(t + (b & 15u), 1u);
        atomicAdd(t + 16, 1u + ((b >> 6) & 1u));
    }
}

// counts [K] = {n_mps, n_redundant}; state [K][maxRow] or null: 0 not counted, 1 counted, 2 counted and redundant
__global__ __launch_bounds__(256) void k_cull_count(const int2 *__restrict__ rows, int nrows, int stride, int maxRow,
                                                    const uint8_t *__restrict__ levels, const uint32_t *__restrict__ mflags,
                                                    int maxPoints, const uint32_t *__restrict__ marks, uint32_t bound,
                                                    const uint32_t *__restrict__ tally, const int2 *__restrict__ cand, int K,
                                                    int monocular, int thObs, int2 *__restrict__ counts, uint8_t *__restrict__ state)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;   // wave-uniform
    const int2 cd = cand[k];
    const bool known = cd.x >= 0 && cd.x < nrows;   // wave-uniform
    const int2 *row = rows + (size_t)(known ? cd.x : 0) * stride;
    const uint8_t *lv = levels + (size_t)(known ? cd.x : 0) * maxRow;
    const int len = known ? min(min(row[0].x, cd.y), maxRow) : 0;
    int nMPs = 0, nRed = 0;
    const int end = state ? maxRow : len;   // (with states the whole [maxRow] segment is written)
    for (int base = 0; base < end; base += 64) {   // (wave-uniform trip count: every lane reaches the sums below)
        const int i = base + lane;
        uint8_t st = 0;
        if (i < len) {
            const int s = kf_entry_slot(row[1 + i], mflags, maxPoints);
            const uint32_t b = lv[i];
            const uint32_t id = s >= 0 ? marks[s] - 1u : 0xFFFFFFFFu;
            if (id < bound && (monocular || !(b & 0x80u))) {
                const uint32_t *t = tally + (size_t)id * CULL_COLS;
                const int top = min((int)(b & 15u) + 1, 15);
                int others = -1;   // the candidate's own entry
#pragma unroll
                for (int o = 0; o < 16; o++) others += o <= top ? (int)t[o] : 0;
                st = ((int)t[16] > thObs && others >= thObs) ? 2 : 1;
            }
        }
        nMPs += st != 0;
        nRed += st == 2;
        if (state && i < maxRow) state[(size_t)k * maxRow + i] = st;
    }
    nMPs = wave_sum(nMPs);
    nRed = wave_sum(nRed);
    if (lane == 0) counts[k] = make_int2(nMPs, nRed);
}

// bytes of m key frames into the level array: desc [m] = {table row, first byte, length}
__global__ __launch_bounds__(256) void k_cull_levels(const uint8_t *__restrict__ bytes, const int32_t *__restrict__ desc, int m,
                                                     int maxKfs, int maxRow, uint8_t *__restrict__ levels)
{
    const int q = blockIdx.x;
    if (q >= m) return;
    const int r = desc[3 * q], off = desc[3 * q + 1], len = min(desc[3 * q + 2], maxRow);
    if (r < 0 || r >= maxKfs || off < 0) return;
    for (int i = threadIdx.x; i < len; i += 256) levels[(size_t)r * maxRow + i] = bytes[off + i];
}

void launch_cull_levels(hipStream_t s, const uint8_t *bytes, const int32_t *desc, int m, int maxKfs, int maxRow, uint8_t *levels)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_cull_levels, dim3(m, 1, 1), dim3(256, 1, 1), 0, s, bytes, desc, m, maxKfs, maxRow, levels);
}

// cand [K] on the device; *nids and tally [bound][17] zeroed on the stream by the caller
void launch_cull(hipStream_t s, const void *rows, int nrows, int stride, int maxRow, const uint8_t *levels, const uint32_t *mflags,
                 int maxPoints, uint32_t *marks, const void *cand, int K, uint32_t bound, uint32_t *nids, uint32_t *tally, int monocular,
                 int thObs, void *counts, uint8_t *state)
{
    if (K <= 0) return;
    const dim3 gk((K + 3) / 4, 1, 1), gr((nrows + 3) / 4, 1, 1), blk(256, 1, 1);
    hipLaunchKernelGGL(k_cull_mark, gk, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, (const int2 *)cand, K, marks,
                       nids);
    if (nrows > 0)
        hipLaunchKernelGGL(k_cull_tally, gr, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, levels, mflags, maxPoints, marks, bound,
                           tally);
    hipLaunchKernelGGL(k_cull_count, gk, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, levels, mflags, maxPoints, marks, bound, tally,
                       (const int2 *)cand, K, monocular, thObs, (int2 *)counts, state);
    hipLaunchKernelGGL(k_cull_clear, gk, blk, 0, s, (const int2 *)rows, nrows, stride, maxRow, mflags, maxPoints, (const int2 *)cand, K, marks);
}
