// api_localmap.hip -- C ABI, part 9: the resident map-point store (orbhip_map_*) and Tracking::SearchLocalPoints as one call
// (orbhip_search_local_points[_device]; kernels in k_localmap.hip and k_guided.hip).  Key -> slot resolution is a host table in
// the context, as for the resident sets: a search resolves its keys while it packs its one upload and costs no device
// synchronisation beyond the one that brings its results back.
#include "api_common.h"

#include "localmap_store.h"

void orb_localmap_release(orbhip_ctx *c)
{
    delete lmap(c);
    c->localMap = nullptr;
}

static void map_reset_table(OrbLocalMap *M)
{
    // every point that was in the store is gone: what a key-frame row still says about its slot must not resolve again
    M->gen.resize(M->maxPoints, 0u);
    M->slotKey.assign(M->maxPoints, 0);
    for (const auto &kv : M->slotOf) M->gen[kv.second]++;
    M->slotOf.clear();
    M->freeSlots.clear();
    M->freeSlots.reserve(M->maxPoints);
    for (int i = M->maxPoints - 1; i >= 0; i--)
        if (M->gen[i] < MP_GEN_END) M->freeSlots.push_back(i);   // (a slot whose generation count is used up is retired)
}

static inline uint32_t map_flag_word(const OrbLocalMap *M, int32_t slot, uint8_t flags)
{
    return MP_LIVE | (flags & (ORBHIP_MP_OBSERVED | ORBHIP_MP_BAD)) | (M->gen[slot] << MP_GEN_SHIFT);
}

extern "C" int orbhip_map_init(orbhip_ctx *c, int max_points)
{
    if (!c || max_points <= 0 || max_points > MAP_MAX_POINTS) return fail(c, ORBHIP_E_ARG, "orbhip_map_init: bad argument");
    HIPCHK(c, orb_enter(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (a queued search may still read the old store)
    orb_localmap_release(c);
    OrbLocalMap *M = new OrbLocalMap();
    M->maxPoints = max_points;
    hipError_t e = M->geoA.grow((size_t)max_points * 16);
    if (e == hipSuccess) e = M->geoB.grow((size_t)max_points * 16);
    if (e == hipSuccess) e = M->flags.grow((size_t)max_points * 4);
    if (e == hipSuccess) e = M->desc.grow((size_t)max_points * 32);
    if (e == hipSuccess) e = hipMemsetAsync(M->flags.as<void>(), 0, (size_t)max_points * 4, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete M;
        return fail(c, ORBHIP_E_HIP, std::string("orbhip_map_init: ") + hipGetErrorString(e));
    }
    map_reset_table(M);
    c->localMap = M;
    return ORBHIP_OK;
}

extern "C" int orbhip_map_clear(orbhip_ctx *c)
{
    if (!c) return ORBHIP_E_ARG;
    OrbLocalMap *M = lmap(c);
    if (!M) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    HIPCHK(c, hipMemsetAsync(M->flags.as<void>(), 0, (size_t)M->maxPoints * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    map_reset_table(M);
    return ORBHIP_OK;
}

extern "C" int orbhip_map_info(orbhip_ctx *c, int *live, int *capacity)
{
    if (!c) return ORBHIP_E_ARG;
    OrbLocalMap *M = lmap(c);
    if (live) *live = M ? (int)M->slotOf.size() : 0;
    if (capacity) *capacity = M ? M->maxPoints : 0;
    return ORBHIP_OK;
}

// a key twice in one call: the scatter kernels write a slot from one lane only
static bool has_duplicates(const uint64_t *keys, int n)
{
    std::vector<uint64_t> k(keys, keys + n);
    std::sort(k.begin(), k.end());
    return std::adjacent_find(k.begin(), k.end()) != k.end();
}

extern "C" int orbhip_map_put(orbhip_ctx *c, int n, const uint64_t *keys, const float *pos, const float *normal,
                              const float *min_dist, const float *max_dist, const uint8_t *desc, const uint8_t *flags)
{
    if (!c || n < 0 || (n > 0 && (!keys || !pos || !normal || !min_dist || !max_dist || !desc || !flags)))
        return fail(c, ORBHIP_E_ARG, "orbhip_map_put: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_map_put: no store (orbhip_map_init)");
    if (n == 0) return ORBHIP_OK;
    size_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (keys[i] == 0) return fail(c, ORBHIP_E_ARG, "orbhip_map_put: key 0");
        if (!M->slotOf.count(keys[i])) fresh++;
    }
    if (has_duplicates(keys, n)) return fail(c, ORBHIP_E_ARG, "orbhip_map_put: a key appears twice");
    if (fresh > M->freeSlots.size()) return fail(c, ORBHIP_E_CAPACITY, "orbhip_map_put: more than max_points map points (orbhip_map_init)");
    HIPCHK(c, orb_enter(c));
    for (int at = 0; at < n; at += MAP_CHUNK) {
        const int m = std::min(MAP_CHUNK, n - at);
        Packed P(c);
        int rc;
        if ((rc = P.begin((size_t)MAP_CHUNK * (4 + 16 + 16 + 4 + 32) + 8 * 256))) return rc;
        int32_t *hs;
        float *ha, *hb;
        uint32_t *hf;
        const int32_t *ds = (const int32_t *)P.in_reserve((size_t)m * 4, (void **)&hs);
        const void *da = P.in_reserve((size_t)m * 16, (void **)&ha);
        const void *db = P.in_reserve((size_t)m * 16, (void **)&hb);
        const uint32_t *df = (const uint32_t *)P.in_reserve((size_t)m * 4, (void **)&hf);
        const void *dd = P.in(desc + (size_t)at * 32, (size_t)m * 32);
        for (int i = 0; i < m; i++) {
            const int g = at + i;
            auto it = M->slotOf.find(keys[g]);
            int32_t s;
            if (it != M->slotOf.end())
                s = it->second;
            else {
                s = M->freeSlots.back();
                M->freeSlots.pop_back();
                M->slotOf.emplace(keys[g], s);
                M->slotKey[s] = keys[g];
            }
            hs[i] = s;
            ha[4 * i] = pos[3 * g], ha[4 * i + 1] = pos[3 * g + 1], ha[4 * i + 2] = pos[3 * g + 2], ha[4 * i + 3] = min_dist[g];
            hb[4 * i] = normal[3 * g], hb[4 * i + 1] = normal[3 * g + 1], hb[4 * i + 2] = normal[3 * g + 2], hb[4 * i + 3] = max_dist[g];
            hf[i] = map_flag_word(M, s, flags[g]);
        }
        if ((rc = P.upload())) return rc;
        launch_map_scatter(c->stream, ds, da, db, df, dd, m, M->maxPoints, M->geoA.as<void>(), M->geoB.as<void>(),
                           M->flags.as<uint32_t>(), M->desc.as<void>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the page-locked block is reused by the next chunk / call)
    }
    return ORBHIP_OK;
}

// flag words of n slots: update_flags (live points) and erase (0)
static int map_write_flags(orbhip_ctx *c, OrbLocalMap *M, const std::vector<int32_t> &slots, const std::vector<uint32_t> &words)
{
    HIPCHK(c, orb_enter(c));
    const int n = (int)slots.size();
    for (int at = 0; at < n; at += MAP_CHUNK) {
        const int m = std::min(MAP_CHUNK, n - at);
        Packed P(c);
        int rc;
        if ((rc = P.begin((size_t)MAP_CHUNK * 8 + 4 * 256))) return rc;
        const int32_t *ds = (const int32_t *)P.in(slots.data() + at, (size_t)m * 4);
        const uint32_t *df = (const uint32_t *)P.in(words.data() + at, (size_t)m * 4);
        if ((rc = P.upload())) return rc;
        launch_map_flags(c->stream, ds, df, m, M->maxPoints, M->flags.as<uint32_t>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_map_update_flags(orbhip_ctx *c, int n, const uint64_t *keys, const uint8_t *flags)
{
    if (!c || n < 0 || (n > 0 && (!keys || !flags))) return fail(c, ORBHIP_E_ARG, "orbhip_map_update_flags: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_map_update_flags: no store (orbhip_map_init)");
    if (n == 0) return ORBHIP_OK;
    std::vector<int32_t> slots(n);
    std::vector<uint32_t> words(n);
    for (int i = 0; i < n; i++) {
        auto it = M->slotOf.find(keys[i]);
        if (it == M->slotOf.end()) return fail(c, ORBHIP_E_ARG, "orbhip_map_update_flags: a key is not in the store");
        slots[i] = it->second;
        words[i] = map_flag_word(M, it->second, flags[i]);
    }
    if (has_duplicates(keys, n)) return fail(c, ORBHIP_E_ARG, "orbhip_map_update_flags: a key appears twice");
    return map_write_flags(c, M, slots, words);
}

extern "C" int orbhip_map_erase(orbhip_ctx *c, int n, const uint64_t *keys)
{
    if (!c || n < 0 || (n > 0 && !keys)) return fail(c, ORBHIP_E_ARG, "orbhip_map_erase: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M || n == 0) return ORBHIP_OK;
    if (has_duplicates(keys, n)) return fail(c, ORBHIP_E_ARG, "orbhip_map_erase: a key appears twice");
    std::vector<int32_t> slots;
    for (int i = 0; i < n; i++) {
        auto it = M->slotOf.find(keys[i]);
        if (it != M->slotOf.end()) slots.push_back(it->second);
    }
    if (slots.empty()) return ORBHIP_OK;
    // the device forgets first: a slot is handed out again only after its flag word is 0
    const int rc = map_write_flags(c, M, slots, std::vector<uint32_t>(slots.size(), 0u));
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        auto it = M->slotOf.find(keys[i]);
        if (it == M->slotOf.end()) continue;
        M->slotKey[it->second] = 0;
        if (++M->gen[it->second] < MP_GEN_END) M->freeSlots.push_back(it->second);
        M->slotOf.erase(it);
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_map_slots(orbhip_ctx *c, int n, const uint64_t *keys, int32_t *slots)
{
    if (!c || n < 0 || (n > 0 && (!keys || !slots))) return fail(c, ORBHIP_E_ARG, "orbhip_map_slots: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_map_slots: no store (orbhip_map_init)");
    for (int i = 0; i < n; i++) {
        auto it = M->slotOf.find(keys[i]);
        slots[i] = it == M->slotOf.end() ? -1 : it->second;
    }
    return ORBHIP_OK;
}

// ---- PredictScale without a device logf: the level is a monotone step function of the ratio ----
static inline float bits_float(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}
static inline bool level_above(float r, float logS, int k) { return logf(r) / logS > (float)k; }   // ceil(x) >= k + 1

// table[k] = the smallest float r with level_above(r, logS, k), k = 0 .. nlevels - 2, by bisection over the bit pattern of the
// positive floats with the host's own logf; false when what that assumes does not hold around the threshold found
static bool build_scale_table(float logS, int nlevels, float *table)
{
    if (!(logS > 0.f) || !std::isfinite(logS) || nlevels < 1 || nlevels > 16) return false;
    for (int k = 0; k < nlevels - 1; k++) {
        uint32_t lo = 0x00800000u, hi = 0x7F7FFFFFu;   // smallest normal, largest finite
        if (level_above(bits_float(lo), logS, k) || !level_above(bits_float(hi), logS, k)) return false;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (level_above(bits_float(mid), logS, k)) hi = mid; else lo = mid;
        }
        for (uint32_t d = 1; d <= 4096; d++)
            if (hi - d >= 0x00800000u && level_above(bits_float(hi - d), logS, k)) return false;
        for (uint32_t d = 0; d < 4096; d++)
            if (hi + d <= 0x7F7FFFFFu && !level_above(bits_float(hi + d), logS, k)) return false;
        if (k > 0 && !(bits_float(hi) >= table[k - 1])) return false;
        table[k] = bits_float(hi);
    }
    return true;
}

extern "C" int orbhip_debug_predict_scale_table(float log_scale_factor, int nlevels, float *table)
{
    if (!table) return ORBHIP_E_ARG;
    float t[15];
    if (!build_scale_table(log_scale_factor, nlevels, t))
        return fail(nullptr, ORBHIP_E_ARG, "orbhip_debug_predict_scale_table: no monotone threshold table for these parameters");
    for (int k = 0; k < nlevels - 1; k++) table[k] = t[k];
    return ORBHIP_OK;
}

extern "C" int orbhip_local_camera_prepare(orbhip_ctx *c, orbhip_local_camera *cam)
{
    if (!c || !cam) return fail(c, ORBHIP_E_ARG, "orbhip_local_camera_prepare: bad argument");
    OrbLocalMap *M = lmap(c);
    float t[15];
    const float *src = t;
    if (M && M->tabValid && M->tabLevels == cam->nlevels && M->tabLogS == cam->log_scale_factor)
        src = M->tab;
    else {
        if (!build_scale_table(cam->log_scale_factor, cam->nlevels, t))
            return fail(c, ORBHIP_E_ARG, "orbhip_local_camera_prepare: no monotone threshold table for log_scale_factor / nlevels");
        if (M) {
            memcpy(M->tab, t, sizeof t);
            M->tabLogS = cam->log_scale_factor;
            M->tabLevels = cam->nlevels;
            M->tabValid = true;
            src = M->tab;
        }
    }
    for (int k = 0; k < 15; k++) cam->level_ratio[k] = k < cam->nlevels - 1 ? src[k] : 0.f;
    cam->reserved = 0;
    return ORBHIP_OK;
}

// ---- the search ----
// frustum kernel -> queries in the matching scratch, behind what the window search carves from it -> window search with the
// store's descriptors read by slot.  d_n_to_match must be zero (zeroIt: a memset node in front).
static int local_points_enqueue(orbhip_ctx *c, OrbLocalMap *M, const void *d_kps, const void *d_desc, const void *d_counts, int cap,
                                int B, const void *d_u_right, const void *d_occupied, float min_x, float min_y, float inv_w,
                                float inv_h, const void *d_cell_off, const void *d_cell_idx, const void *d_cam, const void *d_slots,
                                const void *d_skip, const void *d_nq, int cap_q, float nnratio, void *d_points, void *d_n_to_match,
                                void *d_match, void *d_nmatches, bool zeroIt)
{
    const bool search = d_kps != nullptr;
    const size_t searchBytes = search ? align_up(proj_scratch_bytes(B, cap_q, cap), 256) : 0;
    int rc;
    if ((rc = orb_match_scratch(c, searchBytes + (size_t)B * cap_q * sizeof(orbhip_proj_query) + 256))) return rc;
    orbhip_proj_query *dq = (orbhip_proj_query *)(c->d_match.as<uint8_t>() + searchBytes);
    if (zeroIt) HIPCHK(c, hipMemsetAsync(d_n_to_match, 0, (size_t)B * 4, c->stream));
    launch_local_frustum(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints,
                         (const orbhip_local_camera *)d_cam, (const int32_t *)d_slots, (const uint8_t *)d_skip, (const int32_t *)d_nq,
                         cap_q, B, (orbhip_local_point *)d_points, dq, (int32_t *)d_n_to_match);
    HIPCHK(c, hipGetLastError());
    if (!search) return ORBHIP_OK;
    launch_search_by_projection(c->stream, (const orbhip_keypoint *)d_kps, (const uint8_t *)d_desc, (const int32_t *)d_counts, cap, B,
                                (const float *)d_u_right, (const uint8_t *)d_occupied, min_x, min_y, inv_w, inv_h,
                                (const int32_t *)d_cell_off, (const int32_t *)d_cell_idx, dq, M->desc.as<uint8_t>(),
                                (const int32_t *)d_nq, cap_q, /*use_ratio*/ 1, nnratio, /*check_ori*/ 0, /*TH_HIGH*/ 100,
                                (int32_t *)d_match, (int32_t *)d_nmatches, c->d_match.as<void>(), (const int32_t *)d_slots);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_search_local_points_device(orbhip_ctx *c, const void *d_kps, const void *d_desc, const void *d_counts, int cap,
                                                 int B, const void *d_u_right, const void *d_occupied, float min_x, float min_y,
                                                 float inv_w, float inv_h, const void *d_cell_off, const void *d_cell_idx,
                                                 const void *d_cam, const void *d_slots, const void *d_skip, const void *d_nq,
                                                 int cap_q, float nnratio, void *d_points, void *d_n_to_match, void *d_match,
                                                 void *d_nmatches)
{
    if (!c || !d_kps || !d_desc || !d_counts || cap <= 0 || B <= 0 || !d_cell_off || !d_cell_idx || !d_cam || !d_slots || !d_skip ||
        !d_nq || cap_q <= 0 || !d_points || !d_n_to_match || !d_match || !d_nmatches || !grid_params_ok(inv_w, inv_h) ||
        cap >= (1 << 19))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points_device: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points_device: no store (orbhip_map_init)");
    if (proj_assign_lds(cap) > 120 * 1024)
        return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points_device: cap too large for the per-frame match table in LDS");
    HIPCHK(c, orb_enter(c));
    return local_points_enqueue(c, M, d_kps, d_desc, d_counts, cap, B, d_u_right, d_occupied, min_x, min_y, inv_w, inv_h, d_cell_off,
                                d_cell_idx, d_cam, d_slots, d_skip, d_nq, cap_q, nnratio, d_points, d_n_to_match, d_match, d_nmatches,
                                true);
}

extern "C" int orbhip_search_local_points(orbhip_ctx *c, uint64_t frame_key, const float *u_right, const uint8_t *occupied,
                                          const orbhip_local_camera *cam, const uint64_t *keys, const uint8_t *skip, int nq,
                                          float nnratio, orbhip_local_point *points, int *n_to_match, int32_t *match, int *nmatches)
{
    if (!c || !cam || nq < 0 || (nq > 0 && (!keys || !skip || !points)))
        return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points: no store (orbhip_map_init)");
    OrbSetView S = {};
    if (frame_key != 0) {
        if (!orb_set_grid_view(c, frame_key, &S))
            return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points: unknown set, or a set without a grid (orbhip_set_put)");
        if (!match) return fail(c, ORBHIP_E_ARG, "orbhip_search_local_points: bad argument");
        if (S.n >= (1 << 19) || proj_assign_lds(S.n) > 120 * 1024)
            return fail(c, ORBHIP_E_SIZE, "orbhip_search_local_points: the frame has too many features for the match table in LDS");
    }
    const int n = S.n;
    orbhip_local_camera cm = *cam;
    int rc;
    if ((rc = orbhip_local_camera_prepare(c, &cm))) return rc;
    if (n_to_match) *n_to_match = 0;
    if (nmatches) *nmatches = 0;
    for (int i = 0; i < n; i++) match[i] = -1;
    if (nq == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    if ((rc = P.begin(sizeof cm + (size_t)nq * (4 + 1 + sizeof(orbhip_local_point)) + (size_t)n * (4 + 1 + 4) + 12 * 256))) return rc;
    const void *dcam = P.in(&cm, sizeof cm);
    int32_t *hslots;
    const void *dslots = P.in_reserve((size_t)nq * 4, (void **)&hslots);
    for (int i = 0; i < nq; i++) {
        auto it = M->slotOf.find(keys[i]);
        hslots[i] = it == M->slotOf.end() ? -1 : it->second;
    }
    const void *dskip = P.in(skip, (size_t)nq);
    const float *dur = (n && u_right) ? (const float *)P.in(u_right, (size_t)n * 4) : nullptr;
    const uint8_t *docc = (n && occupied) ? (const uint8_t *)P.in(occupied, (size_t)n) : nullptr;
    const int32_t cnts[4] = {nq, 0, 0, 0};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // nq | points in view | matches (come back with the records and the matches)
    orbhip_local_point *dp = (orbhip_local_point *)P.out((size_t)nq * sizeof(orbhip_local_point));
    int32_t *dm = n ? (int32_t *)P.out((size_t)n * 4) : nullptr;
    if ((rc = P.upload())) return rc;
    if ((rc = local_points_enqueue(c, M, n ? S.d_kps : nullptr, S.d_desc, S.d_cnt, n, 1, dur, docc, S.minX, S.minY, S.invW, S.invH,
                                   S.d_cellOff, S.d_cellIdx, dcam, dslots, dskip, dc, nq, nnratio, dp, dc + 1, dm, dc + 2, false)))
        return rc;
    if ((rc = P.download(dc))) return rc;   // counts | records | matches are adjacent: one copy back, one synchronisation
    memcpy(points, P.host(dp), (size_t)nq * sizeof(orbhip_local_point));
    if (n) memcpy(match, P.host(dm), (size_t)n * 4);
    const int32_t *hc = (const int32_t *)P.host(dc);
    if (n_to_match) *n_to_match = hc[1];
    if (nmatches) *nmatches = n ? hc[2] : 0;
    return ORBHIP_OK;
}

// ---- the key-frame -> map-point table, the covisibility vote and the ordered point union ----
#define KF_NONE (~(uint64_t)0)

static inline uint64_t kf_pack(int32_t slot, uint32_t gen) { return ((uint64_t)gen << 32) | (uint32_t)slot; }
// entry as the device reads it: int2 {slot, generation}, {-1, 0} for no point
static inline void kf_unpack(uint64_t e, int32_t *dst)
{
    dst[0] = e == KF_NONE ? -1 : (int32_t)(uint32_t)e;
    dst[1] = e == KF_NONE ? 0 : (int32_t)(uint32_t)(e >> 32);
}

static void kf_reset_table(OrbKfTable *K)
{
    K->rowOf.clear();
    K->rowHigh = 0;
    K->freeRows.resize(K->maxKfs);
    for (int i = 0; i < K->maxKfs; i++) K->freeRows[i] = K->maxKfs - 1 - i;
    K->rowKey.assign(K->maxKfs, 0);
    K->entries.assign(K->maxKfs, std::vector<uint64_t>());
    K->levelsN.assign(K->maxKfs, -1);
}

extern "C" int orbhip_map_kf_init(orbhip_ctx *c, int max_kfs, int max_row)
{
    if (!c || max_kfs <= 0 || max_kfs > KF_MAX_KFS || max_row <= 0 || max_row > KF_MAX_ROW ||
        (int64_t)max_kfs * (max_row + 1) > KF_MAX_ENTRIES)
        return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_init: bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_init: no store (orbhip_map_init)");
    HIPCHK(c, orb_enter(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    delete M->kf;
    M->kf = nullptr;
    OrbKfTable *K = new OrbKfTable();
    K->maxKfs = max_kfs, K->maxRow = max_row, K->stride = max_row + 1;
    const size_t rowBytes = (size_t)max_kfs * K->stride * 8, slotBytes = (size_t)M->maxPoints * 4;
    hipError_t e = K->rows.grow(rowBytes);
    if (e == hipSuccess) e = K->marks.grow(slotBytes);
    if (e == hipSuccess) e = K->first.grow(slotBytes);
    if (e == hipSuccess) e = hipMemsetAsync(K->rows.as<void>(), 0, rowBytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(K->marks.as<void>(), 0, slotBytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(K->first.as<void>(), 0xFF, slotBytes, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete K;
        return fail(c, ORBHIP_E_HIP, std::string("orbhip_map_kf_init: ") + hipGetErrorString(e));
    }
    kf_reset_table(K);
    M->kf = K;
    return ORBHIP_OK;
}

extern "C" int orbhip_map_kf_clear(orbhip_ctx *c)
{
    if (!c) return ORBHIP_E_ARG;
    OrbKfTable *K = kf_table(c);
    if (!K) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    if (K->rowHigh > 0) HIPCHK(c, hipMemsetAsync(K->rows.as<void>(), 0, (size_t)K->rowHigh * K->stride * 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    kf_reset_table(K);
    return ORBHIP_OK;
}

extern "C" int orbhip_map_kf_info(orbhip_ctx *c, int *live, int *capacity, int *max_row)
{
    if (!c) return ORBHIP_E_ARG;
    OrbKfTable *K = kf_table(c);
    if (live) *live = K ? (int)K->rowOf.size() : 0;
    if (capacity) *capacity = K ? K->maxKfs : 0;
    if (max_row) *max_row = K ? K->maxRow : 0;
    return ORBHIP_OK;
}

// point key -> row entry; false for a key the store does not know
static bool kf_resolve(const OrbLocalMap *M, uint64_t key, uint64_t *e)
{
    if (key == 0) return *e = KF_NONE, true;
    auto it = M->slotOf.find(key);
    if (it == M->slotOf.end()) return false;
    return *e = kf_pack(it->second, M->gen[it->second]), true;
}

// header + entries of one row, from the page-locked block straight into the table
static int kf_upload_row(orbhip_ctx *c, OrbKfTable *K, int row, const std::vector<uint64_t> &ent)
{
    HIPCHK(c, orb_enter(c));
    const int n = (int)ent.size();
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)(n + 1) * 8 + 256))) return rc;
    int32_t *h;
    (void)P.in_reserve((size_t)(n + 1) * 8, (void **)&h);
    h[0] = n, h[1] = 0;
    for (int i = 0; i < n; i++) kf_unpack(ent[i], h + 2 + 2 * i);
    HIPCHK(c, hipMemcpyAsync(K->rows.as<uint8_t>() + (size_t)row * K->stride * 8, h, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (the page-locked block is reused by the next call)
    return ORBHIP_OK;
}

extern "C" int orbhip_map_kf_put(orbhip_ctx *c, uint64_t kf_key, int n, const uint64_t *point_keys)
{
    if (!c || kf_key == 0 || n < 0 || (n > 0 && !point_keys)) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_put: bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_put: no table (orbhip_map_kf_init)");
    if (n > K->maxRow) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_put: more than max_row entries (orbhip_map_kf_init)");
    std::vector<uint64_t> ent(n);
    for (int i = 0; i < n; i++)
        if (!kf_resolve(M, point_keys[i], &ent[i])) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_put: a point key is not in the store");
    {
        std::vector<uint64_t> k;
        for (int i = 0; i < n; i++)
            if (ent[i] != KF_NONE) k.push_back(ent[i]);
        std::sort(k.begin(), k.end());
        if (std::adjacent_find(k.begin(), k.end()) != k.end()) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_put: a point appears twice in the row");
    }
    auto it = K->rowOf.find(kf_key);
    if (it == K->rowOf.end() && K->freeRows.empty())
        return fail(c, ORBHIP_E_CAPACITY, "orbhip_map_kf_put: more than max_kfs key frames (orbhip_map_kf_init)");
    const int row = it != K->rowOf.end() ? it->second : K->freeRows.back();
    int rc;
    if ((rc = kf_upload_row(c, K, row, ent))) return rc;
    if (it == K->rowOf.end()) {
        K->freeRows.pop_back();
        K->rowOf.emplace(kf_key, row);
        K->rowKey[row] = kf_key;
        K->levelsN[row] = -1;   // (another key's levels)
        K->rowHigh = std::max(K->rowHigh, row + 1);
    }
    K->entries[row].swap(ent);
    return ORBHIP_OK;
}

// A point twice in the row `ent` as it will be, idx [m] being the entries that changed (a later entry of the call may have emptied
// the index an earlier one filled: compare what stays).  One pass over the row against the sorted values of the changed indices: a
// Fuse pass sets a hundred entries of a row at a time.
static bool kf_row_twice(const std::vector<uint64_t> &ent, const int32_t *idx, int m)
{
    std::vector<uint8_t> touched(ent.size(), 0);
    std::vector<uint64_t> vals;
    for (int j = 0; j < m; j++) {
        if (touched[idx[j]]) continue;
        touched[idx[j]] = 1;
        if (ent[idx[j]] != KF_NONE) vals.push_back(ent[idx[j]]);
    }
    std::sort(vals.begin(), vals.end());
    bool twice = std::adjacent_find(vals.begin(), vals.end()) != vals.end();
    for (size_t i = 0; i < ent.size() && !twice; i++)
        twice = !touched[i] && ent[i] != KF_NONE && std::binary_search(vals.begin(), vals.end(), ent[i]);
    return twice;
}

extern "C" int orbhip_map_kf_set(orbhip_ctx *c, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys)
{
    if (!c || kf_key == 0 || m < 0 || (m > 0 && (!idx || !point_keys))) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: no table (orbhip_map_kf_init)");
    auto it = K->rowOf.find(kf_key);
    if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: unknown key frame");
    if (m == 0) return ORBHIP_OK;
    const int row = it->second;
    std::vector<uint64_t> ent = K->entries[row];   // the row as it will be
    for (int j = 0; j < m; j++) {
        if (idx[j] < 0 || idx[j] >= (int)ent.size()) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: an index outside the row");
        if (!kf_resolve(M, point_keys[j], &ent[idx[j]])) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: a point key is not in the store");
    }
    if (kf_row_twice(ent, idx, m)) return fail(c, ORBHIP_E_ARG, "orbhip_map_kf_set: a point appears twice in the row");
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)m * 16 + 2 * 256))) return rc;
    int64_t *hat;
    int32_t *hval;
    const int64_t *dat = (const int64_t *)P.in_reserve((size_t)m * 8, (void **)&hat);
    const void *dval = P.in_reserve((size_t)m * 8, (void **)&hval);
    for (int j = 0; j < m; j++) {
        hat[j] = (int64_t)row * K->stride + 1 + idx[j];
        kf_unpack(ent[idx[j]], hval + 2 * j);   // (an index twice in one call: both lanes write the last value)
    }
    if ((rc = P.upload())) return rc;
    launch_kf_set(c->stream, dat, dval, m, (int64_t)K->maxKfs * K->stride, K->rows.as<void>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    K->entries[row].swap(ent);
    return ORBHIP_OK;
}

// orbhip_map_kf_set for entries of many key frames: one upload, one launch, one synchronisation
extern "C" int orbhip_map_kf_set_batch(orbhip_ctx *c, int m, const uint64_t *kf_keys, const int32_t *idx, const uint64_t *point_keys)
{
    const char *who = "orbhip_map_kf_set_batch";
    if (!c || m < 0 || (m > 0 && (!kf_keys || !idx || !point_keys))) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    if (m == 0) return ORBHIP_OK;
    // the entries of each row, in the order of the call
    std::vector<int32_t> rows;                                  // the rows of the call, in order of first appearance
    std::unordered_map<int32_t, std::vector<int32_t> > of;      // row -> the positions j of the call that name it
    for (int j = 0; j < m; j++) {
        auto it = kf_keys[j] ? K->rowOf.find(kf_keys[j]) : K->rowOf.end();
        if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame");
        std::vector<int32_t> &v = of[it->second];
        if (v.empty()) rows.push_back(it->second);
        v.push_back(j);
    }
    std::vector<std::vector<uint64_t> > after(rows.size());     // the rows as they will be
    std::vector<int32_t> ridx;
    for (size_t r = 0; r < rows.size(); r++) {
        std::vector<uint64_t> &ent = after[r];
        ent = K->entries[rows[r]];
        const std::vector<int32_t> &js = of[rows[r]];
        std::vector<uint8_t> named(ent.size(), 0);
        ridx.clear();
        for (int32_t j : js) {
            if (idx[j] < 0 || idx[j] >= (int)ent.size()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": an index outside the row");
            if (named[idx[j]]) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a (key frame, index) pair twice in the call");
            named[idx[j]] = 1;
            if (!kf_resolve(M, point_keys[j], &ent[idx[j]])) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a point key is not in the store");
            ridx.push_back(idx[j]);
        }
        if (kf_row_twice(ent, ridx.data(), (int)ridx.size())) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a point appears twice in a row");
    }
    HIPCHK(c, orb_enter(c));
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)m * 16 + 2 * 256))) return rc;
    int64_t *hat;
    int32_t *hval;
    const int64_t *dat = (const int64_t *)P.in_reserve((size_t)m * 8, (void **)&hat);
    const void *dval = P.in_reserve((size_t)m * 8, (void **)&hval);
    for (size_t r = 0; r < rows.size(); r++)
        for (int32_t j : of[rows[r]]) {
            hat[j] = (int64_t)rows[r] * K->stride + 1 + idx[j];
            kf_unpack(after[r][idx[j]], hval + 2 * j);
        }
    if ((rc = P.upload())) return rc;
    launch_kf_set(c->stream, dat, dval, m, (int64_t)K->maxKfs * K->stride, K->rows.as<void>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t r = 0; r < rows.size(); r++) K->entries[rows[r]].swap(after[r]);
    return ORBHIP_OK;
}

extern "C" int orbhip_map_kf_erase(orbhip_ctx *c, uint64_t kf_key)
{
    if (!c) return ORBHIP_E_ARG;
    OrbKfTable *K = kf_table(c);
    if (!K) return ORBHIP_OK;
    auto it = K->rowOf.find(kf_key);
    if (it == K->rowOf.end()) return ORBHIP_OK;
    const int row = it->second;
    int rc;
    if ((rc = kf_upload_row(c, K, row, std::vector<uint64_t>()))) return rc;   // the device forgets first
    K->entries[row].clear();
    K->rowKey[row] = 0;
    K->levelsN[row] = -1;
    K->freeRows.push_back(row);
    K->rowOf.erase(it);
    return ORBHIP_OK;
}

extern "C" int orbhip_map_vote(orbhip_ctx *c, int n, const uint64_t *frame_point_keys, uint64_t *kf_keys_out, int32_t *counts_out,
                               int cap, int *nout)
{
    if (!c || n < 0 || (n > 0 && !frame_point_keys) || cap < 0 || (cap > 0 && (!kf_keys_out || !counts_out)) || !nout)
        return fail(c, ORBHIP_E_ARG, "orbhip_map_vote: bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_map_vote: no table (orbhip_map_kf_init)");
    *nout = 0;
    if (n == 0 || K->rowHigh == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    const int R = K->rowHigh;
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)n * 4 + 16 + (size_t)R * 8 + 4 * 256))) return rc;
    int32_t *hs;
    const int32_t *ds = (const int32_t *)P.in_reserve((size_t)n * 4, (void **)&hs);
    kf_mark_slots(M, frame_point_keys, n, hs);
    const int32_t zero[4] = {0, 0, 0, 0};
    int32_t *dout = (int32_t *)P.in(zero, 16);   // the count (comes back with the pairs behind it)
    int32_t *dpairs = (int32_t *)P.out((size_t)R * 8);
    if ((rc = P.upload())) return rc;
    launch_mark_add(c->stream, ds, n, M->maxPoints, K->marks.as<uint32_t>());
    launch_vote_rows(c->stream, K->rows.as<void>(), R, K->stride, K->maxRow, M->flags.as<uint32_t>(), M->maxPoints,
                     K->marks.as<uint32_t>(), R, dout, dpairs);
    launch_mark_clear(c->stream, ds, n, M->maxPoints, K->marks.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dout))) return rc;
    const int32_t *h = (const int32_t *)P.host(dpairs);
    const int found = std::min(*(const int32_t *)P.host(dout), R);
    std::vector<std::pair<uint64_t, int32_t> > v;
    v.reserve(found);
    for (int k = 0; k < found; k++) {
        const int row = h[2 * k];
        if (row >= 0 && row < K->maxKfs && K->rowKey[row]) v.push_back(std::make_pair(K->rowKey[row], h[2 * k + 1]));
    }
    std::sort(v.begin(), v.end());   // ascending key: the canonical order of the reference's map<KeyFrame*, int> (docs/parity.md)
    *nout = (int)v.size();
    for (int k = 0; k < (int)v.size() && k < cap; k++) kf_keys_out[k] = v[k].first, counts_out[k] = v[k].second;
    if ((int)v.size() > cap) return fail(c, ORBHIP_E_CAPACITY, "orbhip_map_vote: more key frames than cap (*nout has the number)");
    return ORBHIP_OK;
}

extern "C" int orbhip_map_collect(orbhip_ctx *c, int nkf, const uint64_t *kf_keys, uint64_t *local_keys_out, int cap, int *nlocal)
{
    if (!c || nkf < 0 || (nkf > 0 && !kf_keys) || cap < 0 || (cap > 0 && !local_keys_out) || !nlocal)
        return fail(c, ORBHIP_E_ARG, "orbhip_map_collect: bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_map_collect: no table (orbhip_map_kf_init)");
    *nlocal = 0;
    std::vector<int32_t> rowIdx;
    std::vector<uint32_t> off;
    int rc;
    if ((rc = kf_call_rows(c, K, "orbhip_map_collect", nkf, kf_keys, rowIdx, off))) return rc;
    KfCall Q;
    Q.total = off[nkf];
    if (Q.total == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    const int capOut = (int)std::min<uint64_t>(Q.total, (uint64_t)cap);
    if ((rc = kf_call_scratch(c, K, Q, capOut))) return rc;
    Packed P(c);
    if ((rc = P.begin((size_t)nkf * 8 + 4 + 16 + (size_t)capOut * 4 + 5 * 256))) return rc;
    Q.d_rowIdx = (const int32_t *)P.in(rowIdx.data(), (size_t)nkf * 4);
    Q.d_off = (const uint32_t *)P.in(off.data(), (size_t)(nkf + 1) * 4);
    int32_t *dn = (int32_t *)P.out(256);          // the count | the slots, adjacent: one copy back
    int32_t *dslots = (int32_t *)P.out((size_t)capOut * 4);
    if ((rc = P.upload())) return rc;
    launch_collect(c->stream, K->rows.as<void>(), K->rowHigh, K->stride, Q.d_rowIdx, Q.d_off, nkf, Q.total, M->flags.as<uint32_t>(),
                   M->maxPoints, K->marks.as<uint32_t>(), K->first.as<uint32_t>(), Q.d_cand, Q.d_blockCnt, capOut, dslots, nullptr, dn);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dn))) return rc;
    const int got = *(const int32_t *)P.host(dn);
    const int32_t *hs = (const int32_t *)P.host(dslots);
    *nlocal = got;
    for (int i = 0; i < got && i < capOut; i++) local_keys_out[i] = (hs[i] >= 0 && hs[i] < M->maxPoints) ? M->slotKey[hs[i]] : 0;
    if (got > cap) return fail(c, ORBHIP_E_CAPACITY, "orbhip_map_collect: more local points than cap (*nlocal has the number)");
    return ORBHIP_OK;
}

extern "C" int orbhip_track_local_points(orbhip_ctx *c, uint64_t frame_key, const float *u_right, const uint8_t *occupied,
                                         const orbhip_local_camera *cam, int nkf, const uint64_t *kf_keys, int nseen,
                                         const uint64_t *seen_keys, float nnratio, uint64_t *local_keys_out, int cap, int *nlocal,
                                         orbhip_local_point *points, int *n_to_match, int32_t *match, int *nmatches)
{
    if (!c || !cam || nkf < 0 || (nkf > 0 && !kf_keys) || nseen < 0 || (nseen > 0 && !seen_keys) || cap < 0 ||
        (cap > 0 && (!local_keys_out || !points)) || !nlocal)
        return fail(c, ORBHIP_E_ARG, "orbhip_track_local_points: bad argument");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, "orbhip_track_local_points: no table (orbhip_map_kf_init)");
    OrbSetView S = {};
    if (frame_key != 0) {
        if (!orb_set_grid_view(c, frame_key, &S))
            return fail(c, ORBHIP_E_ARG, "orbhip_track_local_points: unknown set, or a set without a grid (orbhip_set_put)");
        if (!match) return fail(c, ORBHIP_E_ARG, "orbhip_track_local_points: bad argument");
        if (S.n >= (1 << 19) || proj_assign_lds(S.n) > 120 * 1024)
            return fail(c, ORBHIP_E_SIZE, "orbhip_track_local_points: the frame has too many features for the match table in LDS");
    }
    const int n = S.n;
    orbhip_local_camera cm = *cam;
    int rc;
    if ((rc = orbhip_local_camera_prepare(c, &cm))) return rc;
    std::vector<int32_t> rowIdx;
    std::vector<uint32_t> off;
    if ((rc = kf_call_rows(c, K, "orbhip_track_local_points", nkf, kf_keys, rowIdx, off))) return rc;
    *nlocal = 0;
    if (n_to_match) *n_to_match = 0;
    if (nmatches) *nmatches = 0;
    for (int i = 0; i < n; i++) match[i] = -1;
    KfCall Q;
    Q.total = off[nkf];
    const int capQ = (int)std::min<uint64_t>(Q.total, (uint64_t)cap);
    if (Q.total == 0) return ORBHIP_OK;
    if (capQ == 0) {   // nothing can be returned: the count alone
        uint64_t none;
        return orbhip_map_collect(c, nkf, kf_keys, &none, 0, nlocal);
    }
    HIPCHK(c, orb_enter(c));
    if ((rc = kf_call_scratch(c, K, Q, capQ))) return rc;
    Packed P(c);
    if ((rc = P.begin(sizeof cm + (size_t)nkf * 8 + 4 + (size_t)nseen * 4 + (size_t)n * (4 + 1 + 4) +
                      (size_t)capQ * (4 + sizeof(orbhip_local_point)) + 16 * 256)))
        return rc;
    const void *dcam = P.in(&cm, sizeof cm);
    Q.d_rowIdx = (const int32_t *)P.in(rowIdx.data(), (size_t)nkf * 4);
    Q.d_off = (const uint32_t *)P.in(off.data(), (size_t)(nkf + 1) * 4);
    int32_t *hseen;
    const int32_t *dseen = (const int32_t *)P.in_reserve((size_t)nseen * 4, (void **)&hseen);
    kf_mark_slots(M, seen_keys, nseen, hseen);
    const float *dur = (n && u_right) ? (const float *)P.in(u_right, (size_t)n * 4) : nullptr;
    const uint8_t *docc = (n && occupied) ? (const uint8_t *)P.in(occupied, (size_t)n) : nullptr;
    const int32_t cnts[4] = {0, 0, 0, 0};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // local points | points in view | matches (come back with what follows)
    int32_t *dslots = (int32_t *)P.out((size_t)capQ * 4);
    orbhip_local_point *dp = (orbhip_local_point *)P.out((size_t)capQ * sizeof(orbhip_local_point));
    int32_t *dm = n ? (int32_t *)P.out((size_t)n * 4) : nullptr;
    uint8_t *dskip = Q.d_skip;
    if ((rc = P.upload())) return rc;
    uint32_t *marks = K->marks.as<uint32_t>();
    launch_mark_add(c->stream, dseen, nseen, M->maxPoints, marks);
    launch_collect(c->stream, K->rows.as<void>(), K->rowHigh, K->stride, Q.d_rowIdx, Q.d_off, nkf, Q.total, M->flags.as<uint32_t>(),
                   M->maxPoints, marks, K->first.as<uint32_t>(), Q.d_cand, Q.d_blockCnt, capQ, dslots, dskip, dc);
    launch_mark_clear(c->stream, dseen, nseen, M->maxPoints, marks);
    HIPCHK(c, hipGetLastError());
    // the list stays where the union left it: the frustum kernel and the window search read slots, skip bytes and the count there
    if ((rc = local_points_enqueue(c, M, n ? S.d_kps : nullptr, S.d_desc, S.d_cnt, n, 1, dur, docc, S.minX, S.minY, S.invW, S.invH,
                                   S.d_cellOff, S.d_cellIdx, dcam, dslots, dskip, dc, capQ, nnratio, dp, dc + 1, dm, dc + 2, false)))
        return rc;
    if ((rc = P.download(dc))) return rc;   // counts | slots | records | matches: one copy back, one synchronisation
    const int32_t *hc = (const int32_t *)P.host(dc);
    const int32_t *hs = (const int32_t *)P.host(dslots);
    const int got = hc[0];
    *nlocal = got;
    if (got > cap) {
        if (n_to_match) *n_to_match = 0;
        for (int i = 0; i < capQ; i++) local_keys_out[i] = (hs[i] >= 0 && hs[i] < M->maxPoints) ? M->slotKey[hs[i]] : 0;
        return fail(c, ORBHIP_E_CAPACITY, "orbhip_track_local_points: more local points than cap (*nlocal has the number)");
    }
    for (int i = 0; i < got; i++) local_keys_out[i] = (hs[i] >= 0 && hs[i] < M->maxPoints) ? M->slotKey[hs[i]] : 0;
    memcpy(points, P.host(dp), (size_t)got * sizeof(orbhip_local_point));
    if (n) memcpy(match, P.host(dm), (size_t)n * 4);
    if (n_to_match) *n_to_match = hc[1];
    if (nmatches) *nmatches = n ? hc[2] : 0;
    return ORBHIP_OK;
}
