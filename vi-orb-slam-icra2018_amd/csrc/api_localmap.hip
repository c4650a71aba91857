// api_localmap.hip -- C ABI, part 9: the resident map-point store (orbhip_map_*) and Tracking::SearchLocalPoints as one call
// (orbhip_search_local_points[_device]; kernels in k_localmap.hip and k_guided.hip).  Key -> slot resolution is a host table in
// the context, as for the resident sets: a search resolves its keys while it packs its one upload and costs no device
// synchronisation beyond the one that brings its results back.
#include "api_common.h"

#include <unordered_map>

#define MAP_MAX_POINTS (1 << 24)
#define MAP_CHUNK 4096        // points per staged upload of put / update_flags / erase
#define MP_LIVE 0x80u         // (k_localmap.hip)

struct OrbLocalMap {
    int maxPoints = 0;
    OrbBlock geoA, geoB, flags, desc;              // [maxPoints] float4 {P, mfMinDistance} | float4 {normal, mfMaxDistance} | u32 | 32 B
    std::unordered_map<uint64_t, int32_t> slotOf;
    std::vector<int32_t> freeSlots;                // (taken from the back: slot 0 first)
    // the last threshold table (one (mfLogScaleFactor, mnScaleLevels) pair per SLAM session)
    bool tabValid = false;
    float tabLogS = 0.f;
    int tabLevels = 0;
    float tab[15];
};

static OrbLocalMap *lmap(orbhip_ctx *c) { return static_cast<OrbLocalMap *>(c->localMap); }

void orb_localmap_release(orbhip_ctx *c)
{
    delete lmap(c);
    c->localMap = nullptr;
}

static void map_reset_table(OrbLocalMap *M)
{
    M->slotOf.clear();
    M->freeSlots.resize(M->maxPoints);
    for (int i = 0; i < M->maxPoints; i++) M->freeSlots[i] = M->maxPoints - 1 - i;
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
            }
            hs[i] = s;
            ha[4 * i] = pos[3 * g], ha[4 * i + 1] = pos[3 * g + 1], ha[4 * i + 2] = pos[3 * g + 2], ha[4 * i + 3] = min_dist[g];
            hb[4 * i] = normal[3 * g], hb[4 * i + 1] = normal[3 * g + 1], hb[4 * i + 2] = normal[3 * g + 2], hb[4 * i + 3] = max_dist[g];
            hf[i] = MP_LIVE | (flags[g] & (ORBHIP_MP_OBSERVED | ORBHIP_MP_BAD));
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
        words[i] = MP_LIVE | (flags[i] & (ORBHIP_MP_OBSERVED | ORBHIP_MP_BAD));
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
        M->freeSlots.push_back(it->second);
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
