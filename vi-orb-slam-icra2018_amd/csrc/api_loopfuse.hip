// api_loopfuse.hip -- C ABI, part 12: LoopClosing's two projection searches on the resident map.
// orbhip_fuse_sim3: the search half of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ref: src/ORBmatcher.cc:977-1080)
// for all the corrected key frames of LoopClosing::SearchAndFuse (ref: src/LoopClosing.cc:647-673) in one call;
// orbhip_search_loop_points: the union of LoopClosing::ComputeSim3 (ref: :404-424) and SearchByProjection(pKF, Scw, vpPoints,
// vpMatched, th) (ref: src/ORBmatcher.cc:290-403) over it, the list never leaving the device.  The kernels are those of k_fuse.hip
// (the projection with proj_xr = 0, the window search with the chi-square gate off), k_loopfuse.hip ("the key frame holds the point
// already", from the table's rows) and the sequential claim of k_guided.hip.  One packed upload, one dependency chain, one result
// block, one synchronisation; nothing is allocated beyond the grow-only scratch of the context.
#include "localmap_store.h"

extern "C" int orbhip_fuse_sim3(orbhip_ctx *c, const orbhip_fuse_target *targets, const uint64_t *target_row_keys, int K,
                                const uint64_t *point_keys, int n, orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist,
                                int32_t *n_active)
{
    const char *who = "orbhip_fuse_sim3";
    if (!c || K < 0 || n < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (K == 0) return ORBHIP_OK;
    if (!targets || (n > 0 && (!point_keys || !best_idx || !best_dist)) || !n_active)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    OrbKfTable *Kf = kf_table(c);
    std::vector<int32_t> rowIdx(K, -1);
    int maxLen = 0;
    for (int k = 0; k < K && target_row_keys; k++) {
        if (target_row_keys[k] == 0) continue;   // no such test for this target
        if (!Kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
        auto it = Kf->rowOf.find(target_row_keys[k]);
        if (it == Kf->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame (orbhip_map_kf_put)");
        rowIdx[k] = it->second;
        maxLen = std::max(maxLen, (int)Kf->entries[it->second].size());
    }
    FuseTargets T;
    int rc;
    if ((rc = fuse_targets_resolve(c, who, targets, K, T))) return rc;
    if (K > FUSE_MAX_TARGETS || (int64_t)K * n > FUSE_MAX_QUERIES)
        return fail(c, ORBHIP_E_SIZE, std::string(who) + ": more than 65535 targets, or K * n beyond 2^24");
    {   // a key twice: its slot's mark word would have two writers (key 0 is no point and may repeat)
        std::vector<uint64_t> k;
        for (int i = 0; i < n; i++)
            if (point_keys[i]) k.push_back(point_keys[i]);
        std::sort(k.begin(), k.end());
        if (std::adjacent_find(k.begin(), k.end()) != k.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a key twice in point_keys");
    }
    std::vector<orbhip_local_camera> cams(K);
    if ((rc = fuse_cameras_prepare(c, targets, K, cams.data()))) return rc;
    for (int k = 0; k < K; k++) n_active[k] = 0;
    if (n == 0) return ORBHIP_OK;
    const size_t total = (size_t)K * n;
    HIPCHK(c, orb_enter(c));
    // scratch: the targets' feature records | the slot of every (target, point) | the skip bytes | the queries, unless they go back
    const bool held = maxLen > 0;
    const size_t slotBytes = align_up(total * 4, 256), skipBytes = held ? align_up(total, 256) : 0, qBytes = total * sizeof(orbhip_proj_query);
    if ((rc = orb_match_scratch(c, T.recBytes + slotBytes + skipBytes + (queries_out ? 0 : qBytes) + 256))) return rc;
    uint8_t *scratch = c->d_match.as<uint8_t>();
    int32_t *dqslot = (int32_t *)(scratch + T.recBytes);
    uint8_t *dskip = held ? scratch + T.recBytes + slotBytes : nullptr;
    Packed P(c);
    const size_t tb = fuse_target_bytes();
    if ((rc = P.begin((size_t)K * (tb + sizeof(orbhip_local_camera) + 8) + (size_t)n * 4 + total * 8 + qBytes + 12 * 256))) return rc;
    const orbhip_local_camera *dcam = (const orbhip_local_camera *)P.in(cams.data(), (size_t)K * sizeof(orbhip_local_camera));
    const int32_t *drow = (const int32_t *)P.in(rowIdx.data(), (size_t)K * 4);
    int32_t *hslots;
    const int32_t *dslots = (const int32_t *)P.in_reserve((size_t)n * 4, (void **)&hslots);
    kf_mark_slots(M, point_keys, n, hslots);   // -1 for key 0 and for keys the store does not know
    const int32_t cnts[4] = {n, 0, 0, 0};
    const int32_t *dn = (const int32_t *)P.in(cnts, 16);
    const void *dtab = fuse_targets_pack(P, T, scratch, targets, nullptr);
    int32_t *dna = (int32_t *)P.in_fill(0, (size_t)K * 4);   // the active counts (come back with what follows)
    int32_t *dbi = (int32_t *)P.out(total * 4), *dbd = (int32_t *)P.out(total * 4);
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out(qBytes) : (orbhip_proj_query *)(scratch + T.recBytes + slotBytes + skipBytes);
    if ((rc = P.upload())) return rc;
    if (held) {   // spAlreadyFound of every target (:993): the rows' live entries close their points of the list
        HIPCHK(c, hipMemsetAsync(dskip, 0, total, c->stream));
        launch_loop_held(c->stream, Kf->rows.as<void>(), Kf->stride, Kf->maxRow, drow, K, maxLen, M->flags.as<uint32_t>(), M->maxPoints,
                         Kf->marks.as<uint32_t>(), dslots, n, dskip);
    }
    launch_project_fuse_sim3(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints, nullptr, dslots, dn,
                             dskip, dcam, n, K, dq, dqslot, dna);
    launch_window_best_sets(c->stream, dtab, K, T.maxN, dq, M->desc.as<void>(), dqslot, n, dbi, dbd, /*gate*/ false);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dna))) return rc;   // counts | best_idx | best_dist | queries: one copy back, one synchronisation
    memcpy(n_active, P.host(dna), (size_t)K * 4);
    memcpy(best_idx, P.host(dbi), total * 4);
    memcpy(best_dist, P.host(dbd), total * 4);
    if (queries_out) memcpy(queries_out, P.host(dq), qBytes);
    return ORBHIP_OK;
}

extern "C" int orbhip_search_loop_points(orbhip_ctx *c, const orbhip_fuse_target *target, int nkf, const uint64_t *kf_keys,
                                         const uint64_t *matched_keys, int th_high, uint64_t *keys_out, int cap, int *npoints,
                                         orbhip_proj_query *queries_out, int *n_active, int32_t *match, int *nmatches)
{
    const char *who = "orbhip_search_loop_points";
    if (!c || !target || nkf < 0 || (nkf > 0 && !kf_keys) || cap < 0 || (cap > 0 && !keys_out) || !npoints || !n_active || !match ||
        !nmatches)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    OrbKfTable *Kf = kf_table(c);
    if (!Kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    FuseTargets T;
    int rc;
    if ((rc = fuse_targets_resolve(c, who, target, 1, T))) return rc;
    const OrbSetView &S = T.view[0];
    const int n = S.n;
    if (n >= (1 << 19) || proj_assign_lds(n) > 120 * 1024)
        return fail(c, ORBHIP_E_SIZE, std::string(who) + ": the key frame has too many features for the match table in LDS");
    std::vector<int32_t> rowIdx;
    std::vector<uint32_t> off;
    if ((rc = kf_call_rows(c, Kf, who, nkf, kf_keys, rowIdx, off))) return rc;
    orbhip_local_camera cm = target->cam;
    if ((rc = orbhip_local_camera_prepare(c, &cm))) return rc;
    KfCall Q;
    Q.total = off[nkf];
    *npoints = 0;
    *n_active = 0;
    *nmatches = 0;
    for (int i = 0; i < n; i++) match[i] = -1;
    if (Q.total == 0) return ORBHIP_OK;
    const int capQ = (int)std::min<uint64_t>(Q.total, (uint64_t)cap);
    if (capQ == 0) {   // nothing can be returned: the count alone
        uint64_t none;
        return orbhip_map_collect(c, nkf, kf_keys, &none, 0, npoints);
    }
    HIPCHK(c, orb_enter(c));
    if ((rc = kf_call_scratch(c, Kf, Q, capQ))) return rc;
    // scratch: the claim search's | the slot of every point of the list | the queries, unless they go back to the caller
    const bool search = n > 0;
    const size_t searchBytes = search ? align_up(proj_scratch_bytes(1, capQ, n), 256) : 0, slotBytes = align_up((size_t)capQ * 4, 256);
    const size_t qBytes = (size_t)capQ * sizeof(orbhip_proj_query);
    if ((rc = orb_match_scratch(c, searchBytes + slotBytes + (queries_out ? 0 : qBytes) + 256))) return rc;
    int32_t *dqslot = (int32_t *)(c->d_match.as<uint8_t>() + searchBytes);
    Packed P(c);
    if ((rc = P.begin(sizeof cm + (size_t)nkf * 8 + 4 + (size_t)n * (4 + 1 + 4) + (size_t)capQ * 4 + qBytes + 12 * 256))) return rc;
    const orbhip_local_camera *dcam = (const orbhip_local_camera *)P.in(&cm, sizeof cm);
    Q.d_rowIdx = (const int32_t *)P.in(rowIdx.data(), (size_t)nkf * 4);
    Q.d_off = (const uint32_t *)P.in(off.data(), (size_t)(nkf + 1) * 4);
    // vpMatched: its points are inactive (:306-317), its features closed (:375)
    int32_t *hfound = nullptr;
    uint8_t *hocc = nullptr;
    const bool marked = matched_keys && n > 0;
    const int32_t *dfound = marked ? (const int32_t *)P.in_reserve((size_t)n * 4, (void **)&hfound) : nullptr;
    const uint8_t *docc = marked ? (const uint8_t *)P.in_reserve((size_t)n, (void **)&hocc) : nullptr;
    if (marked) {
        kf_mark_slots(M, matched_keys, n, hfound);
        for (int i = 0; i < n; i++) hocc[i] = matched_keys[i] ? 1 : 0;
    }
    const int32_t cnts[4] = {0, 0, 0, 0};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // points | active queries | matches (come back with what follows)
    int32_t *dslots = (int32_t *)P.out((size_t)capQ * 4);
    int32_t *dm = search ? (int32_t *)P.out((size_t)n * 4) : nullptr;
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out(qBytes)
                                        : (orbhip_proj_query *)(c->d_match.as<uint8_t>() + searchBytes + slotBytes);
    if ((rc = P.upload())) return rc;
    uint32_t *marks = Kf->marks.as<uint32_t>();
    launch_collect(c->stream, Kf->rows.as<void>(), Kf->rowHigh, Kf->stride, Q.d_rowIdx, Q.d_off, nkf, Q.total, M->flags.as<uint32_t>(),
                   M->maxPoints, marks, Kf->first.as<uint32_t>(), Q.d_cand, Q.d_blockCnt, capQ, dslots, nullptr, dc);
    if (marked) launch_mark_add(c->stream, dfound, n, M->maxPoints, marks);
    launch_project_fuse_sim3(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints,
                             marked ? marks : nullptr, dslots, dc, nullptr, dcam, capQ, 1, dq, dqslot, dc + 1);
    if (marked) launch_mark_clear(c->stream, dfound, n, M->maxPoints, marks);
    HIPCHK(c, hipGetLastError());
    if (search) {
        launch_search_by_projection(c->stream, S.d_kps, S.d_desc, S.d_cnt, n, 1, nullptr, docc, S.minX, S.minY, S.invW, S.invH,
                                    S.d_cellOff, S.d_cellIdx, dq, M->desc.as<uint8_t>(), dc, capQ, /*use_ratio*/ 0, 0.f,
                                    /*check_ori*/ 0, th_high, dm, dc + 2, c->d_match.as<void>(), dqslot);
        HIPCHK(c, hipGetLastError());
    }
    if ((rc = P.download(dc))) return rc;   // counts | slots | matches | queries: one copy back, one synchronisation
    const int32_t *hc = (const int32_t *)P.host(dc);
    const int got = hc[0];
    *npoints = got;
    if ((rc = collect_keys_out(c, M, (const int32_t *)P.host(dslots), got, capQ, cap, keys_out,
                               std::string(who) + ": more points than cap (*npoints has the number)")))
        return rc;
    *n_active = hc[1];
    if (search) {
        memcpy(match, P.host(dm), (size_t)n * 4);
        *nmatches = hc[2];
    }
    if (queries_out) memcpy(queries_out, P.host(dq), (size_t)got * sizeof(orbhip_proj_query));
    return ORBHIP_OK;
}
