// localmap_store.h -- the host side of the resident map-point store and of the key-frame table, shared by the api_*.hip files
// that search them (api_localmap.hip, api_projtrack.hip, api_fuse.hip): device blocks, the key -> slot / key -> row tables and
// what a call over several rows of the table (the ordered union) sets up.
#ifndef ORBHIP_LOCALMAP_STORE_H
#define ORBHIP_LOCALMAP_STORE_H
#include "api_common.h"
#include "localmap_dev.h"   // MP_LIVE

#include <unordered_map>

#define MAP_MAX_POINTS (1 << 24)
#define MAP_CHUNK 4096        // points per staged upload of put / update_flags / erase
#define MP_GEN_SHIFT 8        // bits 8..31 of a flag word: the slot's generation (k_localcollect.hip)
#define MP_GEN_END (1u << 24)
#define KF_MAX_KFS (1 << 16)
#define KF_MAX_ROW (1 << 13)
#define KF_MAX_ENTRIES ((int64_t)1 << 26)   // 512 MB of rows
#define KF_MAX_CALL (1u << 24)              // row entries per collect: 65536 block counts for the one-block scan

// the key-frame -> map-point table (orbhip_map_kf_*): device rows (k_localcollect.hip) and their host mirror
struct OrbKfTable {
    int maxKfs = 0, maxRow = 0, stride = 0, rowHigh = 0;   // stride = maxRow + 1 entries; rows [0, rowHigh) have been used
    OrbBlock rows, marks, first, scratch;                  // int2 [maxKfs][stride] | u32 [maxPoints] 0 | u32 [maxPoints] ~0 | collect
    std::unordered_map<uint64_t, int32_t> rowOf;
    std::vector<int32_t> freeRows;                         // (taken from the back: row 0 first)
    std::vector<uint64_t> rowKey;                          // [maxKfs] 0 = free
    std::vector<std::vector<uint64_t> > entries;           // [maxKfs] the row as uploaded: generation << 32 | slot, ~0 = no point
};

struct OrbLocalMap {
    int maxPoints = 0;
    OrbBlock geoA, geoB, flags, desc;              // [maxPoints] float4 {P, mfMinDistance} | float4 {normal, mfMaxDistance} | u32 | 32 B
    std::unordered_map<uint64_t, int32_t> slotOf;
    std::vector<int32_t> freeSlots;                // (taken from the back: slot 0 first)
    std::vector<uint32_t> gen;                     // [maxPoints] how often the slot has been freed: bits 8..31 of its flag word
    std::vector<uint64_t> slotKey;                 // [maxPoints] the key in the slot (0 = free)
    OrbKfTable *kf = nullptr;
    ~OrbLocalMap() { delete kf; }
    // the last threshold table (one (mfLogScaleFactor, mnScaleLevels) pair per SLAM session)
    bool tabValid = false;
    float tabLogS = 0.f;
    int tabLevels = 0;
    float tab[15];
};

static inline OrbLocalMap *lmap(orbhip_ctx *c) { return static_cast<OrbLocalMap *>(c->localMap); }
static inline OrbKfTable *kf_table(orbhip_ctx *c) { return lmap(c) ? lmap(c)->kf : nullptr; }

// slots of point keys for the mark scatters: -1 for 0 and for keys the store does not know
static inline void kf_mark_slots(const OrbLocalMap *M, const uint64_t *keys, int n, int32_t *slots)
{
    for (int i = 0; i < n; i++) {
        auto it = keys[i] ? M->slotOf.find(keys[i]) : M->slotOf.end();
        slots[i] = it == M->slotOf.end() ? -1 : it->second;
    }
}

// What a collect needs on the device: the rows of the call and their offsets, uploaded with the caller's block; the scratch
struct KfCall {
    uint32_t total = 0;   // candidates
    const int32_t *d_rowIdx = nullptr;
    const uint32_t *d_off = nullptr;
    int32_t *d_cand = nullptr, *d_blockCnt = nullptr;
    uint8_t *d_skip = nullptr;   // [capOut] (the fused call)
};

// validates the key frames and sizes the candidate list (no device work)
static inline int kf_call_rows(orbhip_ctx *c, OrbKfTable *K, const char *who, int nkf, const uint64_t *kf_keys, std::vector<int32_t> &rowIdx,
                        std::vector<uint32_t> &off)
{
    rowIdx.resize(nkf);
    off.resize(nkf + 1);
    uint64_t total = 0;
    for (int k = 0; k < nkf; k++) {
        auto it = K->rowOf.find(kf_keys[k]);
        if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame");
        rowIdx[k] = it->second;
        off[k] = (uint32_t)total;
        total += K->entries[it->second].size();
        if (total > KF_MAX_CALL) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": more than 2^24 row entries in one call");
    }
    off[nkf] = (uint32_t)total;
    return ORBHIP_OK;
}

static inline int kf_call_scratch(orbhip_ctx *c, OrbKfTable *K, KfCall &Q, int capOut)
{
    const size_t candBytes = align_up((size_t)Q.total * 4, 256), cntBytes = align_up((size_t)collect_blocks(Q.total) * 4, 256);
    const size_t need = candBytes + cntBytes + (size_t)capOut + 256;
    if (K->scratch.bytes() < need) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, K->scratch.grow(need, need + need / 2));
    }
    Q.d_cand = K->scratch.as<int32_t>();
    Q.d_blockCnt = (int32_t *)(K->scratch.as<uint8_t>() + candBytes);
    Q.d_skip = K->scratch.as<uint8_t>() + candBytes + cntBytes;
    return ORBHIP_OK;
}

#endif
