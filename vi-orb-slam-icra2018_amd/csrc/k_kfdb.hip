// k_kfdb.hip -- device half of the key-frame database (KeyFrameDatabase, ref: src/KeyFrameDatabase.cc): the inverted file as a
// CSR over word ids, its rebuild (a stable LSD counting sort of (word, slot) pairs, 8-bit digits) and the query phases of
// DetectLoopCandidates / DetectRelocalizationCandidates for B queries at once.  The host half (slots, delta region, tombstones,
// when to rebuild) is api_kfdb.hip; DESIGN.md "Key-frame database" has the layout and the phases.
//
// Every kernel bounds its own indices (word ids against nwords, query lengths against KFDB_MAX_QWORDS, slots against maxKfs):
// a malformed query sets a status bit and is skipped, it never reads or writes outside the buffers.
#include "orbhip_internal.h"
#include "kfdb_dev.h"

#include <climits>

#define KFDB_TILE_THREADS 256
#define KFDB_TILE_ITEMS 16
#define KFDB_TILE (KFDB_TILE_THREADS * KFDB_TILE_ITEMS)

static __device__ __forceinline__ unsigned long long lanes_below()
{
    const int lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

static __device__ __forceinline__ bool tomb_of(const uint32_t *tomb, uint32_t s) { return (tomb[s >> 5] >> (s & 31)) & 1u; }

// query index of flattened entry g of a CSR with B rows (largest q with off[q] <= g)
static __device__ __forceinline__ int row_of(const int32_t *off, int B, int g)
{
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// slot of `key` in the sorted key map, or -1
static __device__ __forceinline__ int slot_of(const KfdbView &V, uint64_t key)
{
    int lo = 0, hi = V.nmap - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t k = V.mapKey[mid];
        if (k == key) return (int)V.mapSlot[mid];
        if (k < key) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// Exclusive scan of one value per thread over a 256-thread block; `lds` holds 256 ints.  Returns the prefix, `total` the sum.
static __device__ int block_excl_scan(int v, int *lds, int &total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < KFDB_TILE_THREADS; d <<= 1) {
        const int x = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    total = lds[KFDB_TILE_THREADS - 1];
    const int r = lds[t] - v;
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Generic exclusive scan of n ints in place: per-block scans of 2048, a one-block scan of the block sums, the add-back.
__global__ void __launch_bounds__(256) k_scan_blocks(int32_t *a, int n, int32_t *sums)
{
    __shared__ int lds[KFDB_TILE_THREADS];
    const int base = blockIdx.x * 2048 + threadIdx.x * 8;
    int v[8], s = 0;
    for (int k = 0; k < 8; k++) {
        v[k] = base + k < n ? a[base + k] : 0;
        s += v[k];
    }
    int total;
    int run = block_excl_scan(s, lds, total);
    for (int k = 0; k < 8; k++) {
        if (base + k < n) a[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_scan_sums(int32_t *sums, int nb)
{
    __shared__ int lds[KFDB_TILE_THREADS];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += KFDB_TILE_THREADS) {
        const int i = b0 + threadIdx.x;
        const int v = i < nb ? sums[i] : 0;
        int total;
        const int r = block_excl_scan(v, lds, total);
        if (i < nb) sums[i] = carry + r;
        carry += total;
    }
}

__global__ void __launch_bounds__(256) k_scan_add(int32_t *a, int n, const int32_t *sums)
{
    const int base = blockIdx.x * 2048;
    const int add = sums[blockIdx.x];
    for (int k = threadIdx.x; k < 2048; k += KFDB_TILE_THREADS)
        if (base + k < n) a[base + k] += add;
}

// scratch: ceil(n / 2048) ints
void kfdb_scan(hipStream_t s, int32_t *a, int n, int32_t *scratch)
{
    if (n <= 0) return;
    const int nb = (n + 2047) / 2048;
    k_scan_blocks<<<nb, 256, 0, s>>>(a, n, scratch);
    k_scan_sums<<<1, 256, 0, s>>>(scratch, nb);
    k_scan_add<<<nb, 256, 0, s>>>(a, n, scratch);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Rebuild.  The live key frames' BowVectors, in add order, are copied to the new pool; their (word, slot) pairs are then
// sorted by word with a stable LSD counting sort, so that within a word the slots stay in add order (ref: add() push_back).

// one block per live slot: item = {slot, old offset, n, new offset}
__global__ void __launch_bounds__(256) k_fold_expand(const int4 *items, int nitems, const uint32_t *oldW, const double *oldV,
                                                     uint32_t *newW, double *newV, uint32_t *keys, uint32_t *vals)
{
    const int b = blockIdx.x;
    if (b >= nitems) return;
    const int4 it = items[b];
    for (int k = threadIdx.x; k < it.z; k += blockDim.x) {
        const uint32_t w = oldW[(size_t)it.y + k];
        newW[(size_t)it.w + k] = w;
        newV[(size_t)it.w + k] = oldV[(size_t)it.y + k];
        keys[(size_t)it.w + k] = w;
        vals[(size_t)it.w + k] = (uint32_t)it.x;
    }
}

// per tile of KFDB_TILE entries: histogram of the digit, stored digit-major (th[d * ntiles + tile])
__global__ void __launch_bounds__(256) k_radix_hist(const uint32_t *keys, int n, int shift, int ntiles, int32_t *th)
{
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * KFDB_TILE;
    for (int k = 0; k < KFDB_TILE_ITEMS; k++) {
        const size_t i = t0 + (size_t)k * KFDB_TILE_THREADS + threadIdx.x;
        if (i < (size_t)n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    th[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one tile: KFDB_TILE_ITEMS rounds of 256 entries in index order.  Inside a round an entry's rank among the
// equal digits before it comes from the peer mask of its wave (8 ballots) and the counts of the lower waves; `cur` carries the
// tile's running position per digit from round to round.
__global__ void __launch_bounds__(256) k_radix_scatter(const uint32_t *keys, const uint32_t *vals, int n, int shift, int ntiles,
                                                       const int32_t *th, uint32_t *okeys, uint32_t *ovals)
{
    __shared__ int cur[256];
    __shared__ int wcnt[4][256];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    cur[t] = th[(size_t)t * ntiles + blockIdx.x];
    const size_t t0 = (size_t)blockIdx.x * KFDB_TILE;
    for (int r = 0; r < KFDB_TILE_ITEMS; r++) {
        const size_t i = t0 + (size_t)r * KFDB_TILE_THREADS + t;
        const bool valid = i < (size_t)n;
        uint32_t key = 0, val = 0, d = 0;
        if (valid) {
            key = keys[i];
            val = vals[i];
            d = (key >> shift) & 255u;
        }
        wcnt[0][t] = 0;
        wcnt[1][t] = 0;
        wcnt[2][t] = 0;
        wcnt[3][t] = 0;
        __syncthreads();
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const int below = __popcll(peers & lanes_below());
        if (valid && below == 0) wcnt[wave][d] = __popcll(peers);   // the lowest lane of each peer group
        __syncthreads();
        if (valid) {
            int off = cur[d] + below;
            for (int w = 0; w < wave; w++) off += wcnt[w][d];
            okeys[off] = key;
            ovals[off] = val;
        }
        __syncthreads();
        cur[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
        __syncthreads();
        (void)lane;
    }
}

// row[w] = first sorted entry with word >= w, for w in [0, nwords]
__global__ void __launch_bounds__(256) k_rows(const uint32_t *keys, int n, int nwords, uint32_t *row)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nwords) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < (uint32_t)w) lo = mid + 1; else hi = mid;
    }
    row[w] = (uint32_t)lo;
}

// keys/vals hold the n pairs on entry; returns the buffer pair that holds the sorted ones (0: keys/vals, 1: keys2/vals2)
int kfdb_radix_sort(hipStream_t s, uint32_t *keys, uint32_t *vals, uint32_t *keys2, uint32_t *vals2, int n, int nwords,
                    int32_t *th, int32_t *scanScratch)
{
    int bits = 1;
    while (bits < 32 && ((uint32_t)(nwords - 1) >> bits)) bits++;
    const int ntiles = (n + KFDB_TILE - 1) / KFDB_TILE;
    int which = 0;
    for (int shift = 0; shift < bits && n > 0; shift += 8) {
        uint32_t *ik = which ? keys2 : keys, *iv = which ? vals2 : vals;
        uint32_t *ok = which ? keys : keys2, *ov = which ? vals : vals2;
        k_radix_hist<<<ntiles, 256, 0, s>>>(ik, n, shift, ntiles, th);
        kfdb_scan(s, th, 256 * ntiles, scanScratch);
        k_radix_scatter<<<ntiles, 256, 0, s>>>(ik, iv, n, shift, ntiles, th, ok, ov);
        which ^= 1;
    }
    return which;
}

void kfdb_rows(hipStream_t s, const uint32_t *keys, int n, int nwords, uint32_t *row)
{
    k_rows<<<(nwords + 1 + 255) / 256, 256, 0, s>>>(keys, n, nwords, row);
}

static int grid_x(int maxKfs) { return std::max(1, std::min(64, (maxKfs + 255) / 256)); }

// ---------------------------------------------------------------------------------------------------------------------------
// Queries.  Per (query, slot) state lives in B x maxKfs arrays that are zero / all-ones between calls: k_reset puts back what a
// batch touched.

// one block per query: lengths and word order (strictly ascending, < nwords)
__global__ void __launch_bounds__(256) k_q_validate(KfdbView V)
{
    const int q = blockIdx.x;
    const int a = V.qoff[q], n = V.qoff[q + 1] - a;
    if (a < 0 || n < 0 || n > KFDB_MAX_QWORDS) {
        if (threadIdx.x == 0) atomicOr(V.status, KFDB_ST_QLEN);
        return;
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t w = V.qw[a + i];
        if (w >= (uint32_t)V.nwords || (i && V.qw[a + i - 1] >= w)) atomicOr(V.status, KFDB_ST_QWORD);
    }
}

static __device__ __forceinline__ bool q_ok(const KfdbView &V, int q, int &a, int &n)
{
    a = V.qoff[q];
    n = V.qoff[q + 1] - a;
    return a >= 0 && n >= 0 && n <= KFDB_MAX_QWORDS;
}

// excluded keys (flattened CSR over queries) -> excl[q][slot] = val
__global__ void __launch_bounds__(256) k_q_exclude(KfdbView V, int nx, uint8_t val)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nx) return;
    const int q = row_of(V.xoff, V.B, g);
    const int s = slot_of(V, V.xkey[g]);
    if (s >= 0) V.excl[(size_t)q * V.maxKfs + s] = val;
}

// Phase 1 (CSR part): one wave per query word.  Counts shared words per (query, slot), keeps the smallest query-word rank and
// appends a slot to the query's touched list the first time it is met.
__global__ void __launch_bounds__(256) k_q_walk(KfdbView V, int ntotal)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= ntotal) return;
    const int q = row_of(V.qoff, V.B, g);
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const int i = g - a;
    if (i < 0 || i >= n) return;          // only with a malformed qoff (qoff[0] != 0): the host checks it too
    const uint32_t w = V.qw[g];
    if (w >= (uint32_t)V.nwords) return;
    const size_t base = (size_t)q * V.maxKfs;
    for (uint32_t p = V.row[w] + lane; p < V.row[w + 1]; p += 64) {
        const uint32_t s = V.post[p];
        if (tomb_of(V.tomb, s)) continue;
        atomicMin(&V.rank[base + s], (uint32_t)i);
        if (atomicAdd(&V.cnt[base + s], 1) == 0) V.touched[base + atomicAdd(&V.tcount[q], 1)] = (int32_t)s;
    }
}

// two sorted word lists: number of common words and rank (in the query) of the first one
static __device__ int merge_count(const uint32_t *qw, int nq, const uint32_t *kw, int nk, int &first)
{
    int i = 0, j = 0, c = 0;
    first = -1;
    while (i < nq && j < nk) {
        const uint32_t a = qw[i], b = kw[j];
        if (a == b) {
            if (!c) first = i;
            c++;
            i++;
            j++;
        } else if (a < b) {
            i++;
        } else {
            j++;
        }
    }
    return c;
}

// Phase 1 (delta part): thread per (delta slot, query)
__global__ void __launch_bounds__(64) k_q_delta(KfdbView V)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (d >= V.ndelta) return;
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const uint32_t s = (uint32_t)V.delta[d];
    if (tomb_of(V.tomb, s)) return;
    const uint4 m = V.meta[s];
    int first;
    const int c = merge_count(V.qw + a, n, V.poolW + m.x, (int)m.y, first);
    if (!c) return;
    const size_t base = (size_t)q * V.maxKfs;
    V.cnt[base + s] = c;
    V.rank[base + s] = (uint32_t)first;
    V.touched[base + atomicAdd(&V.tcount[q], 1)] = (int32_t)s;
}

// Phase 2: largest shared-word count over the query's non-excluded key frames
__global__ void __launch_bounds__(256) k_q_max(KfdbView V)
{
    const int q = blockIdx.y;
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < tc; t += gridDim.x * blockDim.x) {
        const int s = V.touched[base + t];
        if (!V.excl[base + s]) atomicMax(&V.maxc[q], V.cnt[base + s]);
    }
}

static __device__ __forceinline__ int min_common(int maxc) { return (int)((float)maxc * 0.8f); }   // ref: KeyFrameDatabase.cc:118

// Phase 3: the L1 score (ref: Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-67) of every key frame with more than minCommon
// shared words, as a sequential double sum over the common words in ascending id -- the reference's order, bit for bit.  Also
// counts the touched key frames per first rank (phase 4's bucket sizes).
__global__ void __launch_bounds__(256) k_q_score(KfdbView V)
{
    const int q = blockIdx.y;
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    const int minC = min_common(V.maxc[q]);
    if (blockIdx.x == 0 && threadIdx.x == 0) V.minc[q] = minC;
    const uint32_t *qw = V.qw + a;
    const double *qv = V.qv + a;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < tc; t += gridDim.x * blockDim.x) {
        const int s = V.touched[base + t];
        atomicAdd(&V.cntFirst[(size_t)q * KFDB_MAX_QWORDS + V.rank[base + s]], 1);
        if (V.excl[base + s] || V.cnt[base + s] <= minC) continue;
        const uint4 m = V.meta[s];
        const uint32_t *kw = V.poolW + m.x;
        const double *kv = V.poolV + m.x;
        int i = 0, j = 0;
        const int nk = (int)m.y;
        double score = 0;
        while (i < n && j < nk) {
            const uint32_t x = qw[i], y = kw[j];
            if (x == y) {
                const double vi = qv[i], wi = kv[j];
                score += fabs(vi - wi) - fabs(vi) - fabs(wi);
                i++;
                j++;
            } else if (x < y) {
                i++;
            } else {
                j++;
            }
        }
        score = -score / 2.0;
        V.score[base + s] = (float)score;
    }
}

// Phase 4a: per query, exclusive scan of the bucket sizes over ranks -> start of each rank's run in the ordered list
__global__ void __launch_bounds__(256) k_q_bases(KfdbView V)
{
    __shared__ int lds[KFDB_TILE_THREADS];
    const int q = blockIdx.x;
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    int32_t *cf = V.cntFirst + (size_t)q * KFDB_MAX_QWORDS;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += KFDB_TILE_THREADS) {
        const int i = i0 + threadIdx.x;
        const int v = i < n ? cf[i] : 0;
        int total;
        const int r = block_excl_scan(v, lds, total);
        if (i < n) cf[i] = carry + r;
        carry += total;
    }
}

// Phase 4b (CSR part): one wave per query word i walks the postings of word i again, in add order; the key frames whose first
// shared word is i take consecutive places from the start of rank i's run -- ref order (rank, add sequence).
__global__ void __launch_bounds__(256) k_q_order_csr(KfdbView V, int ntotal)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= ntotal) return;
    const int q = row_of(V.qoff, V.B, g);
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const int i = g - a;
    if (i < 0 || i >= n) return;
    const uint32_t w = V.qw[g];
    if (w >= (uint32_t)V.nwords) return;
    const size_t base = (size_t)q * V.maxKfs;
    const int start = V.cntFirst[(size_t)q * KFDB_MAX_QWORDS + i];
    const uint32_t p0 = V.row[w], p1 = V.row[w + 1];
    int run = 0;
    for (uint32_t pb = p0; pb < p1; pb += 64) {
        const uint32_t p = pb + lane;
        bool mine = false;
        uint32_t s = 0;
        if (p < p1) {
            s = V.post[p];
            mine = !tomb_of(V.tomb, s) && V.rank[base + s] == (uint32_t)i;
        }
        const unsigned long long m = __ballot(mine);
        if (mine) V.ordered[base + start + run + __popcll(m & lanes_below())] = (int32_t)s;
        run += __popcll(m);
    }
    if (lane == 0) V.csrFirst[(size_t)q * KFDB_MAX_QWORDS + i] = run;
}

// Phase 4b (delta part): a delta key frame follows the CSR ones of its rank and the delta ones of that rank added before it
__global__ void __launch_bounds__(64) k_q_order_delta(KfdbView V)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (d >= V.ndelta) return;
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const size_t base = (size_t)q * V.maxKfs;
    const int s = V.delta[d];
    if (tomb_of(V.tomb, (uint32_t)s) || V.cnt[base + s] == 0) return;
    const uint32_t r = V.rank[base + s];
    int local = V.csrFirst[(size_t)q * KFDB_MAX_QWORDS + r];
    for (int e = 0; e < d; e++) {
        const int s2 = V.delta[e];
        if (!tomb_of(V.tomb, (uint32_t)s2) && V.cnt[base + s2] && V.rank[base + s2] == r) local++;
    }
    V.ordered[base + V.cntFirst[(size_t)q * KFDB_MAX_QWORDS + r] + local] = s;
}

// a key frame scored by query b of the batch (the condition of phase 3)
static __device__ __forceinline__ bool scored_by(const KfdbView &V, int b, int s)
{
    const size_t base = (size_t)b * V.maxKfs;
    return V.cnt[base + s] > V.minc[b] && !V.excl[base + s];
}

// Phase 5: covisibility accumulation (ref: KeyFrameDatabase.cc:147-172 loop, :241-268 reloc) for every entry of the ordered
// list that is in lScoreAndMatch.  accBest = -1 marks the others.
__global__ void __launch_bounds__(256) k_q_accumulate(KfdbView V, int reloc, float minScore)
{
    const int q = blockIdx.y;
    int a, n;
    if (!q_ok(V, q, a, n)) return;
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    const int minC = V.minc[q];
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < tc; j += gridDim.x * blockDim.x) {
        const int s = V.ordered[base + j];
        int best = -1;
        float acc = 0.f;
        if (scored_by(V, q, s) && (reloc || V.score[base + s] >= minScore)) {
            float bestScore = V.score[base + s];
            acc = bestScore;
            best = s;
            const int nn = V.nbN[s];
            for (int k = 0; k < nn && k < KFDB_MAX_NEIGH; k++) {
                const int s2 = slot_of(V, V.nbKey[(size_t)s * KFDB_MAX_NEIGH + k]);
                if (s2 < 0 || V.cnt[base + s2] == 0 || V.excl[base + s2]) continue;   // not met by this query
                float v;
                if (V.cnt[base + s2] > minC) {
                    v = V.score[base + s2];
                } else if (reloc) {
                    // mnRelocQuery == F->mnId without a score of this query: the score of the last earlier query that
                    // scored it (this batch first, then the calls before it)
                    v = V.lastReloc[s2];
                    for (int b = q - 1; b >= 0; b--)
                        if (scored_by(V, b, s2)) {
                            v = V.score[(size_t)b * V.maxKfs + s2];
                            break;
                        }
                } else {
                    continue;
                }
                acc += v;
                if (v > bestScore) {
                    best = s2;
                    bestScore = v;
                }
            }
        }
        V.accScore[base + j] = acc;
        V.accBest[base + j] = best;
    }
}

// Phase 6: one block per query.  bestAccScore (ref :174-175 / :269-270), retain accScore > 0.75f * best, keep the first
// occurrence of each pBestKF; the survivors go to cand[q][.] in list order, their number to outCnt[q].
__global__ void __launch_bounds__(256) k_q_retain(KfdbView V, float startBest)
{
    __shared__ int lds[KFDB_TILE_THREADS];
    __shared__ float fmx[KFDB_TILE_THREADS];
    const int q = blockIdx.x;
    int a, n;
    if (!q_ok(V, q, a, n)) {
        if (threadIdx.x == 0) V.outCnt[q] = 0;
        return;
    }
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    float mx = startBest;
    for (int j = threadIdx.x; j < tc; j += blockDim.x)
        if (V.accBest[base + j] >= 0 && V.accScore[base + j] > mx) mx = V.accScore[base + j];
    fmx[threadIdx.x] = mx;
    __syncthreads();
    for (int d = KFDB_TILE_THREADS / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d && fmx[threadIdx.x + d] > fmx[threadIdx.x]) fmx[threadIdx.x] = fmx[threadIdx.x + d];
        __syncthreads();
    }
    const float minRetain = 0.75f * fmx[0];
    for (int j = threadIdx.x; j < tc; j += blockDim.x) {
        const int b = V.accBest[base + j];
        if (b >= 0 && V.accScore[base + j] > minRetain) atomicMin(&V.firstPos[base + b], j);
    }
    __syncthreads();
    int carry = 0;
    for (int j0 = 0; j0 < tc; j0 += KFDB_TILE_THREADS) {
        const int j = j0 + threadIdx.x;
        int b = -1;
        bool keep = false;
        if (j < tc) {
            b = V.accBest[base + j];
            keep = b >= 0 && V.accScore[base + j] > minRetain && V.firstPos[base + b] == j;
        }
        int total;
        const int r = block_excl_scan(keep ? 1 : 0, lds, total);
        if (keep) V.cand[base + carry + r] = b;
        carry += total;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tc; j += blockDim.x) {
        const int b = V.accBest[base + j];
        if (b >= 0) V.firstPos[base + b] = INT_MAX;
    }
    if (threadIdx.x == 0) V.outCnt[q] = carry;
}

// candidates -> keys at the CSR offsets (outOff: exclusive scan of outCnt, B + 1 entries); nothing past outCap is written
__global__ void __launch_bounds__(256) k_q_emit(KfdbView V)
{
    const int q = blockIdx.y;
    const size_t base = (size_t)q * V.maxKfs;
    const int o = V.outOff[q], c = V.outCnt[q];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < c; k += gridDim.x * blockDim.x)
        if (o + k < V.outCap) V.outKeys[o + k] = V.slotKey[V.cand[base + k]];
}

// the single-query result of orbhip_kfdb_score: every key frame met, in the reference's order, with its key, count and score
// (0 where it was not scored); nothing past outCap
__global__ void __launch_bounds__(256) k_q_gather(KfdbView V, int32_t *counts, float *scores)
{
    const int tc = V.tcount[0], minC = V.minc[0];
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < tc && j < V.outCap; j += gridDim.x * blockDim.x) {
        const int s = V.ordered[j];
        V.outKeys[j] = V.slotKey[s];
        counts[j] = V.cnt[s];
        scores[j] = V.cnt[s] > minC && !V.excl[s] ? V.score[s] : 0.f;
    }
}

void kfdb_gather(hipStream_t s, const KfdbView &V, int32_t *counts, float *scores)
{
    k_q_gather<<<grid_x(V.maxKfs), 256, 0, s>>>(V, counts, scores);
}

// reloc: the score a key frame keeps for later queries (KeyFrame::mRelocScore) is the one of the last query in the batch that
// scored it
__global__ void __launch_bounds__(256) k_q_keep_reloc(KfdbView V)
{
    const int q = blockIdx.y;
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < tc; t += gridDim.x * blockDim.x) {
        const int s = V.touched[base + t];
        if (!scored_by(V, q, s)) continue;
        bool later = false;
        for (int b = q + 1; b < V.B && !later; b++) later = scored_by(V, b, s);
        if (!later) V.lastReloc[s] = V.score[base + s];
    }
}

// back to the between-calls state: cnt 0, rank all ones for every slot the batch touched
__global__ void __launch_bounds__(256) k_q_reset(KfdbView V)
{
    const int q = blockIdx.y;
    const size_t base = (size_t)q * V.maxKfs;
    const int tc = V.tcount[q];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < tc; t += gridDim.x * blockDim.x) {
        const int s = V.touched[base + t];
        V.cnt[base + s] = 0;
        V.rank[base + s] = 0xFFFFFFFFu;
    }
}

// out[q + 1] = sum of cnt[0..q], out[0] = 0 (B is small: one block)
__global__ void __launch_bounds__(256) k_q_offsets(const int32_t *cnt, int B, int32_t *out)
{
    __shared__ int lds[KFDB_TILE_THREADS];
    int carry = 0;
    if (threadIdx.x == 0) out[0] = 0;
    for (int q0 = 0; q0 < B; q0 += KFDB_TILE_THREADS) {
        const int q = q0 + threadIdx.x;
        const int v = q < B ? cnt[q] : 0;
        int total;
        const int r = block_excl_scan(v, lds, total);
        if (q < B) out[q + 1] = carry + r + v;
        carry += total;
    }
}

// Phases 1-6 (1-4 with stop_after_order).  ev: KFDB_PHASES + 1 events recorded at the phase boundaries, or null.  Nothing here
// changes the database: the stale reloc scores are committed by kfdb_keep_reloc once the caller knows the call succeeded.
hipError_t kfdb_query_launch(hipStream_t s, const KfdbView &V, int ntotal, int nx, int mode, float minScore,
                             int stop_after_order, hipEvent_t *ev)
{
    const int B = V.B;
    const dim3 per_q(grid_x(V.maxKfs), B);
    const int wblocks = (ntotal + 3) / 4;
    auto mark = [&](int k) {
        if (ev) (void)hipEventRecord(ev[k], s);
    };
    mark(0);
    k_q_validate<<<B, 256, 0, s>>>(V);
    if (nx) k_q_exclude<<<(nx + 255) / 256, 256, 0, s>>>(V, nx, 1);
    if (wblocks) k_q_walk<<<wblocks, 256, 0, s>>>(V, ntotal);
    if (V.ndelta) k_q_delta<<<dim3((V.ndelta + 63) / 64, B), 64, 0, s>>>(V);
    mark(1);
    k_q_max<<<per_q, 256, 0, s>>>(V);
    mark(2);
    k_q_score<<<per_q, 256, 0, s>>>(V);
    mark(3);
    k_q_bases<<<B, 256, 0, s>>>(V);
    if (wblocks) k_q_order_csr<<<wblocks, 256, 0, s>>>(V, ntotal);
    if (V.ndelta) k_q_order_delta<<<dim3((V.ndelta + 63) / 64, B), 64, 0, s>>>(V);
    mark(4);
    if (!stop_after_order) {
        const int reloc = mode == KFDB_MODE_RELOC;
        k_q_accumulate<<<per_q, 256, 0, s>>>(V, reloc, minScore);
        mark(5);
        k_q_retain<<<B, 256, 0, s>>>(V, reloc ? 0.f : minScore);
        k_q_offsets<<<1, 256, 0, s>>>(V.outCnt, B, V.outOff);
        k_q_emit<<<per_q, 256, 0, s>>>(V);
    } else {
        mark(5);
    }
    mark(6);
    return hipGetLastError();
}

// reloc mode, after a successful call: the scores of this batch become the key frames' stale scores (KeyFrame::mRelocScore)
hipError_t kfdb_keep_reloc(hipStream_t s, const KfdbView &V)
{
    k_q_keep_reloc<<<dim3(grid_x(V.maxKfs), V.B), 256, 0, s>>>(V);
    return hipGetLastError();
}

// after the caller has read what it needs: cnt / rank / excl back to their between-calls values
hipError_t kfdb_query_reset(hipStream_t s, const KfdbView &V, int nx)
{
    k_q_reset<<<dim3(grid_x(V.maxKfs), V.B), 256, 0, s>>>(V);
    if (nx) k_q_exclude<<<(nx + 255) / 256, 256, 0, s>>>(V, nx, 0);
    return hipGetLastError();
}

void kfdb_fold_expand(hipStream_t s, const int4 *items, int nitems, const uint32_t *oldW, const double *oldV, uint32_t *newW,
                      double *newV, uint32_t *keys, uint32_t *vals)
{
    if (nitems) k_fold_expand<<<nitems, 256, 0, s>>>(items, nitems, oldW, oldV, newW, newV, keys, vals);
}
