// localmap_store.h -- the host side of the resident map-point store and of the key-frame table, shared by the api_*.hip files
// that search them (api_localmap.hip, api_projtrack.hip, api_fuse.hip, api_loopfuse.hip, api_sim3search.hip, api_refresh.hip,
// api_correct.hip, api_covis.hip, api_cull.hip, api_baproblem.hip, api_bowcand.hip): device blocks, the key -> slot / key -> row
// tables, what a call over several rows of the table (the ordered union) sets up and how it ends, and the target records and
// cameras of the Fuse calls (api_fuse.hip, api_loopfuse.hip, api_sim3search.hip).
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
    OrbBlock levels;                                       // u8 [maxKfs][maxRow], from the first orbhip_map_kf_levels on (api_cull.hip)
    std::vector<int32_t> levelsN;                          // [maxKfs] features the row has levels for, -1 = none
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

// ---- the K target key frames of a Fuse call (api_fuse.hip, api_loopfuse.hip, api_sim3search.hip) ----
#define FUSE_MAX_QUERIES ((int64_t)1 << 24)   // K * n of one call
#define FUSE_MAX_TARGETS 65535                // one target per blockIdx.y
#define FUSE_MAX_SET (1 << 20)                // features of a target set: the row kernel keeps a position in 20 bits

// the per-level tables of a camera record are usable (the frame searches of api_projtrack.hip ask the same)
static inline bool fuse_camera_ok(const orbhip_local_camera *cam) { return cam->nlevels >= 1 && cam->nlevels <= 16 && std::isfinite(cam->th); }

// the K target records of a call, the scratch for their grid-ordered feature records carved behind `recBase`
struct FuseTargets {
    std::vector<OrbSetView> view;
    std::vector<size_t> recOff;   // bytes from the start of the record scratch
    size_t recBytes = 0, urTotal = 0;
    int maxN = 0;
};

static inline int fuse_targets_resolve(orbhip_ctx *c, const char *who, const orbhip_fuse_target *targets, int K, FuseTargets &T)
{
    std::vector<uint64_t> keys;
    for (int k = 0; k < K; k++)
        if (std::find(keys.begin(), keys.end(), targets[k].set_key) == keys.end()) keys.push_back(targets[k].set_key);
    if ((int)keys.size() > orb_set_limit_in_force(c))
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": more distinct sets than the set limit in force (orbhip_set_limit)");
    T.view.resize(K);
    T.recOff.resize(K);
    for (int k = 0; k < K; k++) {
        if (!orb_set_grid_view(c, targets[k].set_key, &T.view[k]))
            return fail(c, ORBHIP_E_ARG, std::string(who) + ": a target is an unknown set, or a set without a grid (orbhip_set_put)");
        if (!fuse_camera_ok(&targets[k].cam)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": nlevels outside 1..16, or th not finite");
    }
    for (int k = 0; k < K; k++) {
        if (T.view[k].n >= FUSE_MAX_SET) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": a target set has 2^20 features or more");
        T.recOff[k] = T.recBytes;
        T.recBytes += align_up((size_t)T.view[k].n * 16, 256);
        T.urTotal += (size_t)T.view[k].n;
        T.maxN = std::max(T.maxN, T.view[k].n);
    }
    return ORBHIP_OK;
}

// cams [K] = the targets' cameras as the projection kernels read them: copied, level_ratio filled (orbhip_local_camera_prepare)
static inline int fuse_cameras_prepare(orbhip_ctx *c, const orbhip_fuse_target *targets, int K, orbhip_local_camera *cams)
{
    for (int k = 0; k < K; k++) {
        cams[k] = targets[k].cam;
        int rc;
        if ((rc = orbhip_local_camera_prepare(c, &cams[k]))) return rc;
    }
    return ORBHIP_OK;
}

// The K records of k_fuse_records and k_window_best_sets in the call's packed block; returns their device twin.  Target k's
// grid-ordered feature records go to recBase + T.recOff[k]; targets[k].inv_level_sigma2 is its gate table; d_uRight = the targets'
// mvuRight one after the other on the device, each as long as its set, or null.
static inline const void *fuse_targets_pack(Packed &P, const FuseTargets &T, uint8_t *recBase, const orbhip_fuse_target *targets,
                                            const float *d_uRight)
{
    const size_t tb = fuse_target_bytes();
    uint8_t *htab;
    const void *dtab = P.in_reserve(T.view.size() * tb, (void **)&htab);
    size_t urAt = 0;
    for (size_t k = 0; k < T.view.size(); k++) {
        const OrbSetView &S = T.view[k];
        fuse_target_fill(htab + k * tb, S.d_kps, S.d_desc, S.d_cellOff, S.d_cellIdx, recBase + T.recOff[k], d_uRight ? d_uRight + urAt : nullptr,
                         S.minX, S.minY, S.invW, S.invH, S.n, targets[k].inv_level_sigma2);
        urAt += (size_t)S.n;
    }
    return dtab;
}

// The tail of a collect: the keys of the slots that came back (0 for one the store does not hold), then ORBHIP_E_CAPACITY with the
// caller's message when there were more than cap.  capQ = min(candidates of the call, cap) slots were written.
static inline int collect_keys_out(orbhip_ctx *c, const OrbLocalMap *M, const int32_t *slots, int got, int capQ, int cap, uint64_t *keys_out,
                                   const std::string &tooMany)
{
    for (int i = 0; i < std::min(got, capQ); i++) keys_out[i] = (slots[i] >= 0 && slots[i] < M->maxPoints) ? M->slotKey[slots[i]] : 0;
    if (got > cap) return fail(c, ORBHIP_E_CAPACITY, tooMany);
    return ORBHIP_OK;
}

#endif
