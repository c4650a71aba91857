// api_kfdb.hip -- C ABI, part 8: the key-frame database (ref: src/KeyFrameDatabase.cc).  A key frame lives in a slot: its
// BowVector in the device pool, its add sequence number in the slot's metadata, its covisibility neighbours (keys) in a table.
// The inverted file is a CSR over word ids holding the slots of every key frame up to the last rebuild; key frames added since
// then sit in a small delta region (a list of slots, in add order), erased ones behind a tombstone bit until the next rebuild
// frees their slot.  A rebuild (fold) runs when the delta region is full or the erased key frames not yet folded out number
// more than max(256, a quarter of the live ones):
// LoopClosing adds one key frame per query, and a rebuild per add would cost a counting sort of the whole file each time.
#include "api_common.h"
#include "kfdb_dev.h"

#include <unordered_map>

struct Kfdb {
    int nwords = 0, maxKfs = 0, deltaMax = 0;
    std::unordered_map<uint64_t, int> slotOf;
    std::vector<uint64_t> slotKey;
    std::vector<uint4> meta;             // pool offset, n, add sequence, 0
    std::vector<uint32_t> tomb;
    std::vector<int> freeSlots;          // popped from the back
    std::vector<int> csr;                // slots in the CSR, add order (tombstoned ones included)
    std::vector<int> delta;              // slots added since the last rebuild, add order
    int ntomb = 0;
    uint32_t seq = 0;
    long long rebuilds = 0;
    bool mapDirty = true, deltaDirty = true;
    int nmap = 0;
    size_t poolUsed = 0, poolCap = 0, pool2Cap = 0, sortCap = 0;
    // device: database
    uint32_t *d_row = nullptr, *d_tomb = nullptr, *d_poolW = nullptr, *d_pool2W = nullptr, *d_post = nullptr;
    double *d_poolV = nullptr, *d_pool2V = nullptr;
    uint4 *d_meta = nullptr;
    uint64_t *d_nbKey = nullptr, *d_mapKey = nullptr, *d_slotKey = nullptr;
    uint8_t *d_nbN = nullptr;
    uint32_t *d_mapSlot = nullptr;
    float *d_lastReloc = nullptr;
    int32_t *d_delta = nullptr;
    // device: rebuild scratch
    uint32_t *d_keys[2] = {nullptr, nullptr}, *d_vals[2] = {nullptr, nullptr};
    int32_t *d_th = nullptr, *d_scan = nullptr;
    size_t thCap = 0, scanCap = 0;
    int4 *d_items = nullptr;
    // device: per-batch state for up to capB queries
    int capB = 0;
    int32_t *d_cnt = nullptr, *d_firstPos = nullptr, *d_touched = nullptr, *d_ordered = nullptr, *d_accBest = nullptr,
            *d_cand = nullptr, *d_cntFirst = nullptr, *d_csrFirst = nullptr, *d_small = nullptr;
    uint32_t *d_rank = nullptr;
    float *d_score = nullptr, *d_accScore = nullptr;
    uint8_t *d_excl = nullptr;
    // orbhip_kfdb_set_timing: events at the phase boundaries of every query call, the last call's phase times
    hipEvent_t ev[KFDB_PHASES + 1] = {};
    bool timing = false;
    float phaseMs[KFDB_PHASES] = {};
};

static void dfree(void *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}
template <class T>
static void dfree(T *&p)
{
    void *v = p;
    dfree(v);
    p = nullptr;
}

static void batch_free(Kfdb *K)
{
    dfree(K->d_cnt), dfree(K->d_firstPos), dfree(K->d_touched), dfree(K->d_ordered), dfree(K->d_accBest), dfree(K->d_cand);
    dfree(K->d_cntFirst), dfree(K->d_csrFirst), dfree(K->d_small), dfree(K->d_rank), dfree(K->d_score), dfree(K->d_accScore);
    dfree(K->d_excl);
    K->capB = 0;
}

static void kfdb_free(Kfdb *K)
{
    batch_free(K);
    dfree(K->d_row), dfree(K->d_tomb), dfree(K->d_poolW), dfree(K->d_pool2W), dfree(K->d_post), dfree(K->d_poolV);
    dfree(K->d_pool2V), dfree(K->d_meta), dfree(K->d_nbKey), dfree(K->d_mapKey), dfree(K->d_slotKey), dfree(K->d_nbN);
    dfree(K->d_mapSlot), dfree(K->d_lastReloc), dfree(K->d_delta), dfree(K->d_keys[0]), dfree(K->d_keys[1]);
    dfree(K->d_vals[0]), dfree(K->d_vals[1]), dfree(K->d_th), dfree(K->d_scan), dfree(K->d_items);
    for (hipEvent_t &e : K->ev)
        if (e) (void)hipEventDestroy(e);
    delete K;
}

void orb_kfdb_release(orbhip_ctx *c)
{
    if (!c->kfdb) return;
    kfdb_free(static_cast<Kfdb *>(c->kfdb));
    c->kfdb = nullptr;
}

template <class T>
static int dalloc(orbhip_ctx *c, T *&p, size_t count)
{
    void *v = nullptr;
    HIPCHK(c, hipMalloc(&v, count ? count * sizeof(T) : 16));
    p = static_cast<T *>(v);
    return ORBHIP_OK;
}

#define KCHK(expr)                    \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_) return rc_;          \
    } while (0)

static Kfdb *db(orbhip_ctx *c) { return c ? static_cast<Kfdb *>(c->kfdb) : nullptr; }

// a slot becomes free for a new key frame only once nothing of it is left in the CSR (at a rebuild for erased ones)
static void reset_slots(Kfdb *K)
{
    K->freeSlots.resize(K->maxKfs);
    for (int i = 0; i < K->maxKfs; i++) K->freeSlots[i] = K->maxKfs - 1 - i;
    K->slotOf.clear();
    std::fill(K->tomb.begin(), K->tomb.end(), 0u);
    K->csr.clear();
    K->delta.clear();
    K->ntomb = 0;
    K->poolUsed = 0;
    K->mapDirty = K->deltaDirty = true;
}

extern "C" int orbhip_kfdb_init(orbhip_ctx *c, int nwords, int max_kfs, int delta_max)
{
    if (!c) return ORBHIP_E_ARG;
    if (nwords < 1 || max_kfs < 1 || max_kfs > (1 << 22) || delta_max < 0 || delta_max > 4096)
        return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_init: nwords >= 1, 1 <= max_kfs <= 4194304, 0 <= delta_max <= 4096");
    HIPCHK(c, orb_enter(c));
    orb_kfdb_release(c);
    Kfdb *K = new Kfdb();
    c->kfdb = K;
    K->nwords = nwords;
    K->maxKfs = max_kfs;
    K->deltaMax = delta_max ? delta_max : 128;
    K->slotKey.assign(max_kfs, 0);
    K->meta.assign(max_kfs, make_uint4(0, 0, 0, 0));
    K->tomb.assign((max_kfs + 31) / 32, 0u);
    reset_slots(K);
    const size_t M = (size_t)max_kfs;
    KCHK(dalloc(c, K->d_row, (size_t)nwords + 1));
    KCHK(dalloc(c, K->d_tomb, K->tomb.size()));
    KCHK(dalloc(c, K->d_meta, M));
    KCHK(dalloc(c, K->d_nbKey, M * KFDB_MAX_NEIGH));
    KCHK(dalloc(c, K->d_nbN, M));
    KCHK(dalloc(c, K->d_mapKey, M));
    KCHK(dalloc(c, K->d_mapSlot, M));
    KCHK(dalloc(c, K->d_slotKey, M));
    KCHK(dalloc(c, K->d_lastReloc, M));
    KCHK(dalloc(c, K->d_delta, (size_t)K->deltaMax));
    KCHK(dalloc(c, K->d_post, 1));
    HIPCHK(c, hipMemsetAsync(K->d_row, 0, ((size_t)nwords + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_tomb, 0, K->tomb.size() * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_nbN, 0, M, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_lastReloc, 0, M * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

// the pool holds at least `need` entries (appends between rebuilds; a rebuild compacts it)
static int pool_reserve(orbhip_ctx *c, Kfdb *K, size_t need)
{
    if (need <= K->poolCap) return ORBHIP_OK;
    const size_t cap = std::max(need, std::max((size_t)1 << 16, K->poolCap * 2));
    uint32_t *w = nullptr;
    double *v = nullptr;
    KCHK(dalloc(c, w, cap));
    if (dalloc(c, v, cap)) {
        dfree(w);
        return ORBHIP_E_HIP;
    }
    if (K->poolUsed) {
        HIPCHK(c, hipMemcpyAsync(w, K->d_poolW, K->poolUsed * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(v, K->d_poolV, K->poolUsed * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    dfree(K->d_poolW);
    dfree(K->d_poolV);
    K->d_poolW = w;
    K->d_poolV = v;
    K->poolCap = cap;
    return ORBHIP_OK;
}

template <class T>
static int grow(orbhip_ctx *c, T *&p, size_t &cap, size_t need)
{
    if (need <= cap && p) return ORBHIP_OK;
    dfree(p);
    cap = 0;
    const size_t n = std::max(need + need / 4, (size_t)4096);
    KCHK(dalloc(c, p, n));
    cap = n;
    return ORBHIP_OK;
}

// Rebuild: the live key frames (CSR ones not erased, then the delta region -- add order) are copied to a compacted pool, their
// (word, slot) pairs sorted by word (stable), the CSR rows recomputed.  Erased slots become free.
static int fold(orbhip_ctx *c, Kfdb *K)
{
    std::vector<int> live;
    live.reserve(K->csr.size() + K->delta.size());
    for (int s : K->csr) {
        if ((K->tomb[s >> 5] >> (s & 31)) & 1u)
            K->freeSlots.push_back(s);
        else
            live.push_back(s);
    }
    for (int s : K->delta) live.push_back(s);
    std::vector<int4> items(live.size());
    size_t total = 0;
    for (size_t i = 0; i < live.size(); i++) {
        const int s = live[i];
        items[i] = make_int4(s, (int)K->meta[s].x, (int)K->meta[s].y, (int)total);
        K->meta[s].x = (uint32_t)total;
        total += K->meta[s].y;
    }
    if (total > (size_t)INT32_MAX - (1 << 20)) return fail(c, ORBHIP_E_CAPACITY, "orbhip_kfdb: inverted file beyond 2^31 entries");
    size_t cap = K->pool2Cap;
    if (total > cap || !K->d_pool2W) {
        dfree(K->d_pool2W);
        dfree(K->d_pool2V);
        cap = std::max(total + total / 4, (size_t)1 << 16);
        KCHK(dalloc(c, K->d_pool2W, cap));
        KCHK(dalloc(c, K->d_pool2V, cap));
        K->pool2Cap = cap;
    }
    if (total > K->sortCap || !K->d_keys[0]) {
        for (int b = 0; b < 2; b++) dfree(K->d_keys[b]), dfree(K->d_vals[b]);
        K->sortCap = std::max(total + total / 4, (size_t)1 << 16);
        for (int b = 0; b < 2; b++) {
            KCHK(dalloc(c, K->d_keys[b], K->sortCap));
            KCHK(dalloc(c, K->d_vals[b], K->sortCap));
        }
    }
    const size_t ntiles = (total + 4095) / 4096;
    KCHK(grow(c, K->d_th, K->thCap, 256 * ntiles + 1));
    KCHK(grow(c, K->d_scan, K->scanCap, (256 * ntiles + 2047) / 2048 + 1));
    dfree(K->d_items);
    KCHK(dalloc(c, K->d_items, items.size()));
    if (!items.empty())
        HIPCHK(c, hipMemcpyAsync(K->d_items, items.data(), items.size() * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    kfdb_fold_expand(c->stream, K->d_items, (int)items.size(), K->d_poolW, K->d_poolV, K->d_pool2W, K->d_pool2V, K->d_keys[0],
                     K->d_vals[0]);
    const int which = kfdb_radix_sort(c->stream, K->d_keys[0], K->d_vals[0], K->d_keys[1], K->d_vals[1], (int)total, K->nwords,
                                      K->d_th, K->d_scan);
    kfdb_rows(c->stream, K->d_keys[which], (int)total, K->nwords, K->d_row);
    HIPCHK(c, hipGetLastError());
    // the sorted slots are the postings; the other value buffer is scratch for the next rebuild
    std::swap(K->d_post, K->d_vals[which]);
    std::swap(K->d_poolW, K->d_pool2W);
    std::swap(K->d_poolV, K->d_pool2V);
    std::swap(K->poolCap, K->pool2Cap);
    K->poolUsed = total;
    std::fill(K->tomb.begin(), K->tomb.end(), 0u);
    HIPCHK(c, hipMemsetAsync(K->d_tomb, 0, K->tomb.size() * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_meta, K->meta.data(), K->meta.size() * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // d_post's old buffer went to d_vals[which] (of any size): a fresh scratch buffer of sortCap entries takes its place
    dfree(K->d_vals[which]);
    KCHK(dalloc(c, K->d_vals[which], K->sortCap));
    K->csr = live;
    K->delta.clear();
    K->ntomb = 0;
    K->rebuilds++;
    K->deltaDirty = true;
    return ORBHIP_OK;
}

static int check_bow(orbhip_ctx *c, const Kfdb *K, const uint32_t *word, const double *value, int n, const char *who)
{
    if (n < 0 || (n && (!word || !value))) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad BowVector pointers");
    if (n > KFDB_MAX_QWORDS)
        return fail(c, ORBHIP_E_SIZE, std::string(who) + ": more than 8192 words in one BowVector");
    for (int i = 0; i < n; i++)
        if (word[i] >= (uint32_t)K->nwords || (i && word[i - 1] >= word[i]))
            return fail(c, ORBHIP_E_ARG, std::string(who) + ": word ids must be strictly ascending and below nwords");
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_add(orbhip_ctx *c, uint64_t key, const uint32_t *word, const double *value, int n)
{
    Kfdb *K = db(c);
    if (!K) return c ? fail(c, ORBHIP_E_ARG, "orbhip_kfdb_add: no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    KCHK(check_bow(c, K, word, value, n, "orbhip_kfdb_add"));
    if (K->slotOf.count(key)) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_add: key already in the database");
    HIPCHK(c, orb_enter(c));
    if (K->freeSlots.empty() && K->ntomb) KCHK(fold(c, K));
    if (K->freeSlots.empty()) return fail(c, ORBHIP_E_CAPACITY, "orbhip_kfdb_add: database full (max_kfs key frames)");
    KCHK(pool_reserve(c, K, K->poolUsed + (size_t)n));
    const int s = K->freeSlots.back();
    K->freeSlots.pop_back();
    K->meta[s] = make_uint4((uint32_t)K->poolUsed, (uint32_t)n, K->seq++, 0);
    K->slotKey[s] = key;
    const float zero = 0.f;
    const uint8_t none = 0;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(K->d_poolW + K->poolUsed, word, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(K->d_poolV + K->poolUsed, value, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(K->d_meta + s, &K->meta[s], sizeof(uint4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_slotKey + s, &key, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_lastReloc + s, &zero, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_nbN + s, &none, 1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    K->poolUsed += (size_t)n;
    K->slotOf[key] = s;
    K->delta.push_back(s);
    K->mapDirty = K->deltaDirty = true;
    if ((int)K->delta.size() >= K->deltaMax) KCHK(fold(c, K));
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_erase(orbhip_ctx *c, uint64_t key)
{
    Kfdb *K = db(c);
    if (!K) return c ? fail(c, ORBHIP_E_ARG, "orbhip_kfdb_erase: no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    auto it = K->slotOf.find(key);
    if (it == K->slotOf.end()) return ORBHIP_OK;   // ref: erase of a key frame that is not in the file changes nothing
    HIPCHK(c, orb_enter(c));
    const int s = it->second;
    K->slotOf.erase(it);
    K->mapDirty = true;
    auto d = std::find(K->delta.begin(), K->delta.end(), s);
    if (d != K->delta.end()) {
        K->delta.erase(d);
        K->freeSlots.push_back(s);
        K->deltaDirty = true;
        return ORBHIP_OK;
    }
    K->tomb[s >> 5] |= 1u << (s & 31);
    K->ntomb++;
    HIPCHK(c, hipMemcpyAsync(K->d_tomb + (s >> 5), &K->tomb[s >> 5], 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (K->ntomb > std::max(256, (int)K->slotOf.size() / 4)) KCHK(fold(c, K));
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_clear(orbhip_ctx *c)
{
    Kfdb *K = db(c);
    if (!K) return c ? fail(c, ORBHIP_E_ARG, "orbhip_kfdb_clear: no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    HIPCHK(c, orb_enter(c));
    reset_slots(K);
    HIPCHK(c, hipMemsetAsync(K->d_row, 0, ((size_t)K->nwords + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_tomb, 0, K->tomb.size() * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_set_covis(orbhip_ctx *c, uint64_t key, const uint64_t *neigh, int n)
{
    Kfdb *K = db(c);
    if (!K) return c ? fail(c, ORBHIP_E_ARG, "orbhip_kfdb_set_covis: no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    if (n < 0 || n > KFDB_MAX_NEIGH || (n && !neigh))
        return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_set_covis: 0 <= n <= 10 neighbours");
    auto it = K->slotOf.find(key);
    if (it == K->slotOf.end()) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_set_covis: key not in the database");
    HIPCHK(c, orb_enter(c));
    const int s = it->second;
    const uint8_t nn = (uint8_t)n;
    if (n)
        HIPCHK(c, hipMemcpyAsync(K->d_nbKey + (size_t)s * KFDB_MAX_NEIGH, neigh, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_nbN + s, &nn, 1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_info(orbhip_ctx *c, int *live, int *delta, int *tombs, long long *rebuilds)
{
    Kfdb *K = db(c);
    if (!K) return ORBHIP_E_ARG;
    if (live) *live = (int)K->slotOf.size();
    if (delta) *delta = (int)K->delta.size();
    if (tombs) *tombs = K->ntomb;
    if (rebuilds) *rebuilds = K->rebuilds;
    return ORBHIP_OK;
}

// per-batch arrays for B queries; between calls cnt = 0, rank = all ones, excl = 0, firstPos = large
static int batch_reserve(orbhip_ctx *c, Kfdb *K, int B)
{
    if (B <= K->capB) return ORBHIP_OK;
    batch_free(K);
    const size_t BM = (size_t)B * K->maxKfs, BQ = (size_t)B * KFDB_MAX_QWORDS;
    KCHK(dalloc(c, K->d_cnt, BM));
    KCHK(dalloc(c, K->d_rank, BM));
    KCHK(dalloc(c, K->d_score, BM));
    KCHK(dalloc(c, K->d_excl, BM));
    KCHK(dalloc(c, K->d_firstPos, BM));
    KCHK(dalloc(c, K->d_touched, BM));
    KCHK(dalloc(c, K->d_ordered, BM));
    KCHK(dalloc(c, K->d_accScore, BM));
    KCHK(dalloc(c, K->d_accBest, BM));
    KCHK(dalloc(c, K->d_cand, BM));
    KCHK(dalloc(c, K->d_cntFirst, BQ));
    KCHK(dalloc(c, K->d_csrFirst, BQ));
    KCHK(dalloc(c, K->d_small, (size_t)B * 5 + 8));
    HIPCHK(c, hipMemsetAsync(K->d_cnt, 0, BM * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_rank, 0xFF, BM * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_excl, 0, BM, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_firstPos, 0x7F, BM * 4, c->stream));
    K->capB = B;
    return ORBHIP_OK;
}

// uploads what changed since the last query (key map, delta list) and fills the database half of the view
static int prepare(orbhip_ctx *c, Kfdb *K, int B, KfdbView &V)
{
    if (K->mapDirty) {
        std::vector<std::pair<uint64_t, int>> m(K->slotOf.begin(), K->slotOf.end());
        std::sort(m.begin(), m.end());
        std::vector<uint64_t> keys(m.size());
        std::vector<uint32_t> slots(m.size());
        for (size_t i = 0; i < m.size(); i++) keys[i] = m[i].first, slots[i] = (uint32_t)m[i].second;
        if (!m.empty()) {
            HIPCHK(c, hipMemcpyAsync(K->d_mapKey, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(K->d_mapSlot, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        K->nmap = (int)m.size();
        K->mapDirty = false;
    }
    if (K->deltaDirty) {
        if (!K->delta.empty())
            HIPCHK(c, hipMemcpyAsync(K->d_delta, K->delta.data(), K->delta.size() * 4, hipMemcpyHostToDevice, c->stream));
        K->deltaDirty = false;
    }
    KCHK(batch_reserve(c, K, B));
    V.nwords = K->nwords;
    V.maxKfs = K->maxKfs;
    V.row = K->d_row;
    V.post = K->d_post;
    V.tomb = K->d_tomb;
    V.meta = K->d_meta;
    V.poolW = K->d_poolW;
    V.poolV = K->d_poolV;
    V.delta = K->d_delta;
    V.ndelta = (int)K->delta.size();
    V.nbKey = K->d_nbKey;
    V.nbN = K->d_nbN;
    V.mapKey = K->d_mapKey;
    V.mapSlot = K->d_mapSlot;
    V.nmap = K->nmap;
    V.slotKey = K->d_slotKey;
    V.lastReloc = K->d_lastReloc;
    V.B = B;
    V.cnt = K->d_cnt;
    V.rank = K->d_rank;
    V.score = K->d_score;
    V.excl = K->d_excl;
    V.firstPos = K->d_firstPos;
    V.touched = K->d_touched;
    V.ordered = K->d_ordered;
    V.accScore = K->d_accScore;
    V.accBest = K->d_accBest;
    V.cand = K->d_cand;
    V.cntFirst = K->d_cntFirst;
    V.csrFirst = K->d_csrFirst;
    V.tcount = K->d_small;
    V.maxc = K->d_small + B;
    V.minc = K->d_small + 2 * B;
    V.outCnt = K->d_small + 3 * B;
    V.status = K->d_small + 4 * B;
    HIPCHK(c, hipMemsetAsync(K->d_small, 0, ((size_t)B * 5 + 8) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_cntFirst, 0, (size_t)B * KFDB_MAX_QWORDS * 4, c->stream));
    return ORBHIP_OK;
}

static int status_error(orbhip_ctx *c, int st, const char *who)
{
    if (st & KFDB_ST_QLEN)
        return fail(c, ORBHIP_E_SIZE, std::string(who) + ": a query has more than 8192 words (or qoff does not ascend from 0)");
    if (st & KFDB_ST_QWORD)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": query word ids must be strictly ascending and below nwords");
    return ORBHIP_OK;
}

static int check_mode(orbhip_ctx *c, Kfdb *K, int mode, const char *who)
{
    if (!K) return c ? fail(c, ORBHIP_E_ARG, std::string(who) + ": no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    if (mode != ORBHIP_KFDB_RELOC && mode != ORBHIP_KFDB_LOOP)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": mode is ORBHIP_KFDB_RELOC or ORBHIP_KFDB_LOOP");
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_set_timing(orbhip_ctx *c, int on)
{
    Kfdb *K = db(c);
    if (!K) return c ? fail(c, ORBHIP_E_ARG, "orbhip_kfdb_set_timing: no database (orbhip_kfdb_init)") : ORBHIP_E_ARG;
    HIPCHK(c, orb_enter(c));
    if (on)
        for (hipEvent_t &e : K->ev)
            if (!e) HIPCHK(c, hipEventCreate(&e));
    K->timing = on != 0;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_phase_times(orbhip_ctx *c, float *ms)
{
    Kfdb *K = db(c);
    if (!K || !ms) return ORBHIP_E_ARG;
    for (int k = 0; k < KFDB_PHASES; k++) ms[k] = K->phaseMs[k];
    return ORBHIP_OK;
}

static void read_phase_times(Kfdb *K)
{
    for (int k = 0; k < KFDB_PHASES; k++)
        if (hipEventElapsedTime(&K->phaseMs[k], K->ev[k], K->ev[k + 1]) != hipSuccess) K->phaseMs[k] = 0.f;
}

// The end of every query call, once its results are on the host (the stream is idle): in reloc mode a call that succeeded
// commits its scores as the stale scores of later queries -- a call that fails (an invalid query, too small an output) leaves
// the database as it was, so that calling again with a larger output gives what B sequential calls give.  Then the per-batch
// state goes back to its between-calls values.
static int finish(orbhip_ctx *c, Kfdb *K, const KfdbView &V, int mode, int nx, bool ok)
{
    if (K->timing) read_phase_times(K);
    if (ok && mode == ORBHIP_KFDB_RELOC) HIPCHK(c, kfdb_keep_reloc(c->stream, V));
    HIPCHK(c, kfdb_query_reset(c->stream, V, nx));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_score(orbhip_ctx *c, int mode, const uint32_t *word, const double *value, int n,
                                 const uint64_t *excluded, int nx, uint64_t *keys, int32_t *counts, float *scores, int cap,
                                 int *nout, int *min_common)
{
    Kfdb *K = db(c);
    KCHK(check_mode(c, K, mode, "orbhip_kfdb_score"));
    KCHK(check_bow(c, K, word, value, n, "orbhip_kfdb_score"));
    if (nx < 0 || (nx && !excluded) || cap < 0 || (cap && (!keys || !counts || !scores)) || !nout)
        return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_score: bad arguments");
    HIPCHK(c, orb_enter(c));
    KfdbView V;
    KCHK(prepare(c, K, 1, V));
    Packed P(c);
    const int32_t qoff[2] = {0, n}, xoff[2] = {0, nx};
    KCHK(P.begin(16 + (size_t)n * 12 + (size_t)nx * 8 + (size_t)cap * 16 + 4096));
    V.qoff = (const int32_t *)P.in(qoff, 8);
    V.qw = (const uint32_t *)P.in(word, (size_t)n * 4);
    V.qv = (const double *)P.in(value, (size_t)n * 8);
    V.xoff = (const int32_t *)P.in(xoff, 8);
    V.xkey = (const uint64_t *)P.in(excluded, (size_t)nx * 8);
    uint64_t *dk = (uint64_t *)P.out((size_t)cap * 8);
    int32_t *dc = (int32_t *)P.out((size_t)cap * 4);
    float *ds = (float *)P.out((size_t)cap * 4);
    int32_t *dsmall = (int32_t *)P.out(16);
    V.outKeys = dk;
    V.outCap = cap;
    KCHK(P.upload());
    HIPCHK(c, kfdb_query_launch(c->stream, V, n, nx, mode, 0.f, 1, K->timing ? K->ev : nullptr));
    kfdb_gather(c->stream, V, dc, ds);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dsmall, V.tcount, 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dsmall + 1, V.minc, 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dsmall + 2, V.status, 4, hipMemcpyDeviceToDevice, c->stream));
    KCHK(P.download());
    const int32_t *hs = (const int32_t *)P.host(dsmall);
    KCHK(finish(c, K, V, mode, nx, hs[2] == 0 && hs[0] <= cap));
    KCHK(status_error(c, hs[2], "orbhip_kfdb_score"));
    *nout = hs[0];
    if (min_common) *min_common = hs[1];
    const int m = std::min(hs[0], cap);
    if (m) {
        memcpy(keys, P.host(dk), (size_t)m * 8);
        memcpy(counts, P.host(dc), (size_t)m * 4);
        memcpy(scores, P.host(ds), (size_t)m * 4);
    }
    if (hs[0] > cap) return fail(c, ORBHIP_E_CAPACITY, "orbhip_kfdb_score: more key frames share a word than cap");
    return ORBHIP_OK;
}

// The batch on device pointers; qtotal / nx: qoff[B] / xoff[B] as the host knows them.  The status word and out_off[B] go to
// tail_dst[0..1] (device or page-locked memory); the caller reads them after a synchronisation and calls finish().
static int detect_launch(orbhip_ctx *c, Kfdb *K, KfdbView &V, int mode, int B, const int32_t *qoff, const uint32_t *qw,
                         const double *qv, const int32_t *xoff, const uint64_t *xkey, int qtotal, int nx, float min_score,
                         int32_t *out_off, uint64_t *out_keys, int out_cap, int32_t *tail_dst)
{
    KCHK(prepare(c, K, B, V));
    V.qoff = qoff;
    V.qw = qw;
    V.qv = qv;
    V.xoff = xoff;
    V.xkey = xkey;
    V.outOff = out_off;
    V.outKeys = out_keys;
    V.outCap = out_cap;
    HIPCHK(c, kfdb_query_launch(c->stream, V, qtotal, nx, mode, min_score, 0, K->timing ? K->ev : nullptr));
    HIPCHK(c, hipMemcpyAsync(tail_dst, V.status, 4, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(tail_dst + 1, out_off + B, 4, hipMemcpyDefault, c->stream));
    return ORBHIP_OK;
}

static int check_batch(orbhip_ctx *c, int B, int out_cap, const char *who)
{
    if (B < 1 || B > KFDB_MAX_BATCH) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": 1 <= B <= 1024 queries");
    if (out_cap < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": out_cap < 0");
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_detect(orbhip_ctx *c, int mode, int B, const int32_t *qoff, const uint32_t *qword,
                                  const double *qvalue, const int32_t *xoff, const uint64_t *xkey, float min_score,
                                  int32_t *out_off, uint64_t *out_keys, int out_cap)
{
    Kfdb *K = db(c);
    KCHK(check_mode(c, K, mode, "orbhip_kfdb_detect"));
    KCHK(check_batch(c, B, out_cap, "orbhip_kfdb_detect"));
    if (!qoff || !out_off || (out_cap && !out_keys)) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect: null pointer");
    if (qoff[0] != 0) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect: qoff[0] != 0");
    for (int q = 0; q < B; q++) {
        KCHK(check_bow(c, K, qword + qoff[q], qvalue + qoff[q], qoff[q + 1] - qoff[q], "orbhip_kfdb_detect"));
        if (xoff && xoff[q + 1] < xoff[q]) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect: xoff not ascending");
    }
    const int qt = qoff[B];
    std::vector<int32_t> xzero;
    if (!xoff) xzero.assign(B + 1, 0), xoff = xzero.data();
    if (xoff[0] != 0 || (xoff[B] && !xkey)) return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect: bad excluded keys");
    const int nx = xoff[B];
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    KCHK(P.begin((size_t)(B + 1) * 8 + (size_t)qt * 12 + (size_t)nx * 8 + (size_t)out_cap * 8 + (size_t)(B + 1) * 4 + 4096));
    const int32_t *dqo = (const int32_t *)P.in(qoff, (size_t)(B + 1) * 4);
    const uint32_t *dqw = (const uint32_t *)P.in(qword, (size_t)qt * 4);
    const double *dqv = (const double *)P.in(qvalue, (size_t)qt * 8);
    const int32_t *dxo = (const int32_t *)P.in(xoff, (size_t)(B + 1) * 4);
    const uint64_t *dxk = (const uint64_t *)P.in(xkey, (size_t)nx * 8);
    int32_t *doff = (int32_t *)P.out((size_t)(B + 1) * 4);
    uint64_t *dkeys = (uint64_t *)P.out((size_t)out_cap * 8);
    int32_t *dtail = (int32_t *)P.out(8);
    KCHK(P.upload());
    KfdbView V;
    KCHK(detect_launch(c, K, V, mode, B, dqo, dqw, dqv, dxo, dxk, qt, nx, min_score, doff, dkeys, out_cap, dtail));
    KCHK(P.download());
    const int32_t *tail = (const int32_t *)P.host(dtail);
    KCHK(finish(c, K, V, mode, nx, tail[0] == 0 && tail[1] <= out_cap));
    KCHK(status_error(c, tail[0], "orbhip_kfdb_detect"));
    memcpy(out_off, P.host(doff), (size_t)(B + 1) * 4);
    const int total = out_off[B];
    if (total > out_cap) return fail(c, ORBHIP_E_CAPACITY, "orbhip_kfdb_detect: more candidates than out_cap (out_off is filled)");
    if (total) memcpy(out_keys, P.host(dkeys), (size_t)total * 8);
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_detect_device(orbhip_ctx *c, int mode, int B, const void *d_qoff, const void *d_qword,
                                         const void *d_qvalue, const void *d_xoff, const void *d_xkey, float min_score,
                                         void *d_out_off, void *d_out_keys, int out_cap)
{
    Kfdb *K = db(c);
    KCHK(check_mode(c, K, mode, "orbhip_kfdb_detect_device"));
    KCHK(check_batch(c, B, out_cap, "orbhip_kfdb_detect_device"));
    if (!d_qoff || !d_xoff || !d_out_off || (out_cap && !d_out_keys))
        return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect_device: null pointer");
    HIPCHK(c, orb_enter(c));
    if (orb_host_stage(c, 64)) return ORBHIP_E_HIP;
    int32_t *h = (int32_t *)c->h_stage;   // qoff[0] | qoff[B] | xoff[0] | xoff[B] | status | out_off[B]
    HIPCHK(c, hipMemcpyAsync(h + 0, d_qoff, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 1, (const int32_t *)d_qoff + B, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 2, d_xoff, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h + 3, (const int32_t *)d_xoff + B, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h[0] != 0 || h[1] < 0 || h[2] != 0 || h[3] < 0 || (h[3] && !d_xkey))
        return fail(c, ORBHIP_E_ARG, "orbhip_kfdb_detect_device: qoff / xoff must start at 0 and end at a size >= 0");
    const int qt = h[1], nx = h[3];
    KfdbView V;
    KCHK(detect_launch(c, K, V, mode, B, (const int32_t *)d_qoff, (const uint32_t *)d_qword, (const double *)d_qvalue,
                       (const int32_t *)d_xoff, (const uint64_t *)d_xkey, qt, nx, min_score, (int32_t *)d_out_off,
                       (uint64_t *)d_out_keys, out_cap, h + 4));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int st = h[4], total = h[5];
    KCHK(finish(c, K, V, mode, nx, st == 0 && total <= out_cap));
    KCHK(status_error(c, st, "orbhip_kfdb_detect_device"));
    if (total > out_cap)
        return fail(c, ORBHIP_E_CAPACITY, "orbhip_kfdb_detect_device: more candidates than out_cap (out_off is filled)");
    return ORBHIP_OK;
}
