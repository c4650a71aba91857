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
    size_t poolUsed = 0;                 // entries of the pool in use (its capacity is d_poolW's)
    // device: database (element types in the comments)
    OrbBlock d_row, d_tomb, d_poolW, d_pool2W, d_post;   // uint32_t
    OrbBlock d_poolV, d_pool2V;                          // double
    OrbBlock d_meta;                                     // uint4
    OrbBlock d_nbKey, d_mapKey, d_slotKey;               // uint64_t
    OrbBlock d_nbN;                                      // uint8_t
    OrbBlock d_mapSlot;                                  // uint32_t
    OrbBlock d_lastReloc;                                // float
    OrbBlock d_delta;                                    // int32_t
    // device: rebuild scratch
    OrbBlock d_keys[2], d_vals[2];                       // uint32_t
    OrbBlock d_th, d_scan;                               // int32_t
    OrbBlock d_items;                                    // int4
    // device: per-batch state for up to capB queries
    int capB = 0;
    OrbBlock d_cnt, d_firstPos, d_touched, d_ordered, d_accBest, d_cand, d_cntFirst, d_csrFirst, d_small;   // int32_t
    OrbBlock d_rank;                                     // uint32_t
    OrbBlock d_score, d_accScore;                        // float
    OrbBlock d_excl;                                     // uint8_t
    // orbhip_kfdb_set_timing: events at the phase boundaries of every query call, the last call's phase times
    hipEvent_t ev[KFDB_PHASES + 1] = {};
    bool timing = false;
    float phaseMs[KFDB_PHASES] = {};
};

void orb_kfdb_release(orbhip_ctx *c)
{
    Kfdb *K = static_cast<Kfdb *>(c->kfdb);
    if (!K) return;
    for (hipEvent_t &e : K->ev)
        if (e) (void)hipEventDestroy(e);
    delete K;
    c->kfdb = nullptr;
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
    HIPCHK(c, K->d_row.grow(((size_t)nwords + 1) * 4));
    HIPCHK(c, K->d_tomb.grow(K->tomb.size() * 4));
    HIPCHK(c, K->d_meta.grow(M * sizeof(uint4)));
    HIPCHK(c, K->d_nbKey.grow(M * KFDB_MAX_NEIGH * 8));
    HIPCHK(c, K->d_nbN.grow(M));
    HIPCHK(c, K->d_mapKey.grow(M * 8));
    HIPCHK(c, K->d_mapSlot.grow(M * 4));
    HIPCHK(c, K->d_slotKey.grow(M * 8));
    HIPCHK(c, K->d_lastReloc.grow(M * 4));
    HIPCHK(c, K->d_delta.grow((size_t)K->deltaMax * 4));
    HIPCHK(c, K->d_post.grow(4));
    HIPCHK(c, hipMemsetAsync(K->d_row.as<uint32_t>(), 0, ((size_t)nwords + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_tomb.as<uint32_t>(), 0, K->tomb.size() * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_nbN.as<uint8_t>(), 0, M, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_lastReloc.as<float>(), 0, M * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

// the pool holds at least `need` entries (appends between rebuilds; a rebuild compacts it)
static int pool_reserve(orbhip_ctx *c, Kfdb *K, size_t need)
{
    const size_t poolCap = K->d_poolW.bytes() / 4;
    if (need <= poolCap) return ORBHIP_OK;
    const size_t cap = std::max(need, std::max((size_t)1 << 16, poolCap * 2));
    OrbBlock w, v;
    HIPCHK(c, w.grow(cap * 4));
    HIPCHK(c, v.grow(cap * 8));
    if (K->poolUsed) {
        HIPCHK(c, hipMemcpyAsync(w.as<void>(), K->d_poolW.as<void>(), K->poolUsed * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(v.as<void>(), K->d_poolV.as<void>(), K->poolUsed * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    K->d_poolW = std::move(w);
    K->d_poolV = std::move(v);
    return ORBHIP_OK;
}

// entries of slack: what a rebuild buffer of `n` entries is allocated with
static size_t slack(size_t n, size_t floor) { return std::max(n + n / 4, floor); }

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
    const size_t cap = slack(total, (size_t)1 << 16);   // entries of the compacted pool and the sort buffers when they grow
    HIPCHK(c, K->d_pool2W.grow(total * 4, cap * 4));
    HIPCHK(c, K->d_pool2V.grow(total * 8, cap * 8));
    for (int b = 0; b < 2; b++) {
        HIPCHK(c, K->d_keys[b].grow(total * 4, cap * 4));
        HIPCHK(c, K->d_vals[b].grow(total * 4, cap * 4));
    }
    const size_t ntiles = (total + 4095) / 4096, nth = 256 * ntiles + 1, nscan = (256 * ntiles + 2047) / 2048 + 1;
    HIPCHK(c, K->d_th.grow(nth * 4, slack(nth, 4096) * 4));
    HIPCHK(c, K->d_scan.grow(nscan * 4, slack(nscan, 4096) * 4));
    K->d_items.reset();
    HIPCHK(c, K->d_items.grow(items.size() * sizeof(int4)));
    if (!items.empty())
        HIPCHK(c, hipMemcpyAsync(K->d_items.as<int4>(), items.data(), items.size() * sizeof(int4), hipMemcpyHostToDevice,
                                 c->stream));
    kfdb_fold_expand(c->stream, K->d_items.as<int4>(), (int)items.size(), K->d_poolW.as<uint32_t>(), K->d_poolV.as<double>(),
                     K->d_pool2W.as<uint32_t>(), K->d_pool2V.as<double>(), K->d_keys[0].as<uint32_t>(),
                     K->d_vals[0].as<uint32_t>());
    const int which = kfdb_radix_sort(c->stream, K->d_keys[0].as<uint32_t>(), K->d_vals[0].as<uint32_t>(),
                                      K->d_keys[1].as<uint32_t>(), K->d_vals[1].as<uint32_t>(), (int)total, K->nwords,
                                      K->d_th.as<int32_t>(), K->d_scan.as<int32_t>());
    kfdb_rows(c->stream, K->d_keys[which].as<uint32_t>(), (int)total, K->nwords, K->d_row.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    // the sorted slots are the postings; the other value buffer is scratch for the next rebuild
    std::swap(K->d_post, K->d_vals[which]);
    std::swap(K->d_poolW, K->d_pool2W);
    std::swap(K->d_poolV, K->d_pool2V);
    K->poolUsed = total;
    std::fill(K->tomb.begin(), K->tomb.end(), 0u);
    HIPCHK(c, hipMemsetAsync(K->d_tomb.as<uint32_t>(), 0, K->tomb.size() * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_meta.as<uint4>(), K->meta.data(), K->meta.size() * sizeof(uint4), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // d_post's old buffer went to d_vals[which] (of any size): a fresh scratch buffer as large as the others takes its place
    K->d_vals[which].reset();
    HIPCHK(c, K->d_vals[which].grow(K->d_keys[which].bytes()));
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
        HIPCHK(c, hipMemcpyAsync(K->d_poolW.as<uint32_t>() + K->poolUsed, word, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(K->d_poolV.as<double>() + K->poolUsed, value, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(K->d_meta.as<uint4>() + s, &K->meta[s], sizeof(uint4), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_slotKey.as<uint64_t>() + s, &key, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_lastReloc.as<float>() + s, &zero, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_nbN.as<uint8_t>() + s, &none, 1, hipMemcpyHostToDevice, c->stream));
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
    HIPCHK(c, hipMemcpyAsync(K->d_tomb.as<uint32_t>() + (s >> 5), &K->tomb[s >> 5], 4, hipMemcpyHostToDevice, c->stream));
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
    HIPCHK(c, hipMemsetAsync(K->d_row.as<uint32_t>(), 0, ((size_t)K->nwords + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_tomb.as<uint32_t>(), 0, K->tomb.size() * 4, c->stream));
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
        HIPCHK(c, hipMemcpyAsync(K->d_nbKey.as<uint64_t>() + (size_t)s * KFDB_MAX_NEIGH, neigh, (size_t)n * 8,
                                 hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(K->d_nbN.as<uint8_t>() + s, &nn, 1, hipMemcpyHostToDevice, c->stream));
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
    K->capB = 0;
    const size_t BM = (size_t)B * K->maxKfs, BQ = (size_t)B * KFDB_MAX_QWORDS;
    for (OrbBlock *b : {&K->d_cnt, &K->d_rank, &K->d_score, &K->d_firstPos, &K->d_touched, &K->d_ordered, &K->d_accScore,
                        &K->d_accBest, &K->d_cand})
        HIPCHK(c, b->grow(BM * 4));
    HIPCHK(c, K->d_excl.grow(BM));
    HIPCHK(c, K->d_cntFirst.grow(BQ * 4));
    HIPCHK(c, K->d_csrFirst.grow(BQ * 4));
    HIPCHK(c, K->d_small.grow(((size_t)B * 5 + 8) * 4));
    HIPCHK(c, hipMemsetAsync(K->d_cnt.as<int32_t>(), 0, BM * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_rank.as<uint32_t>(), 0xFF, BM * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_excl.as<uint8_t>(), 0, BM, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_firstPos.as<int32_t>(), 0x7F, BM * 4, c->stream));
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
            HIPCHK(c, hipMemcpyAsync(K->d_mapKey.as<uint64_t>(), keys.data(), keys.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(K->d_mapSlot.as<uint32_t>(), slots.data(), slots.size() * 4, hipMemcpyHostToDevice,
                                     c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        K->nmap = (int)m.size();
        K->mapDirty = false;
    }
    if (K->deltaDirty) {
        if (!K->delta.empty())
            HIPCHK(c, hipMemcpyAsync(K->d_delta.as<int32_t>(), K->delta.data(), K->delta.size() * 4, hipMemcpyHostToDevice,
                                     c->stream));
        K->deltaDirty = false;
    }
    KCHK(batch_reserve(c, K, B));
    V.nwords = K->nwords;
    V.maxKfs = K->maxKfs;
    V.row = K->d_row.as<uint32_t>();
    V.post = K->d_post.as<uint32_t>();
    V.tomb = K->d_tomb.as<uint32_t>();
    V.meta = K->d_meta.as<uint4>();
    V.poolW = K->d_poolW.as<uint32_t>();
    V.poolV = K->d_poolV.as<double>();
    V.delta = K->d_delta.as<int32_t>();
    V.ndelta = (int)K->delta.size();
    V.nbKey = K->d_nbKey.as<uint64_t>();
    V.nbN = K->d_nbN.as<uint8_t>();
    V.mapKey = K->d_mapKey.as<uint64_t>();
    V.mapSlot = K->d_mapSlot.as<uint32_t>();
    V.nmap = K->nmap;
    V.slotKey = K->d_slotKey.as<uint64_t>();
    V.lastReloc = K->d_lastReloc.as<float>();
    V.B = B;
    V.cnt = K->d_cnt.as<int32_t>();
    V.rank = K->d_rank.as<uint32_t>();
    V.score = K->d_score.as<float>();
    V.excl = K->d_excl.as<uint8_t>();
    V.firstPos = K->d_firstPos.as<int32_t>();
    V.touched = K->d_touched.as<int32_t>();
    V.ordered = K->d_ordered.as<int32_t>();
    V.accScore = K->d_accScore.as<float>();
    V.accBest = K->d_accBest.as<int32_t>();
    V.cand = K->d_cand.as<int32_t>();
    V.cntFirst = K->d_cntFirst.as<int32_t>();
    V.csrFirst = K->d_csrFirst.as<int32_t>();
    V.tcount = K->d_small.as<int32_t>();
    V.maxc = K->d_small.as<int32_t>() + B;
    V.minc = K->d_small.as<int32_t>() + 2 * B;
    V.outCnt = K->d_small.as<int32_t>() + 3 * B;
    V.status = K->d_small.as<int32_t>() + 4 * B;
    HIPCHK(c, hipMemsetAsync(K->d_small.as<int32_t>(), 0, ((size_t)B * 5 + 8) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(K->d_cntFirst.as<int32_t>(), 0, (size_t)B * KFDB_MAX_QWORDS * 4, c->stream));
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
    int32_t *h = (int32_t *)c->h_stage.as<uint8_t>();   // qoff[0] | qoff[B] | xoff[0] | xoff[B] | status | out_off[B]
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
