// api_fuse.hip -- C ABI, part 11: ORBmatcher::Fuse(pKF, vpMapPoints, th) for LocalMapping::SearchInNeighbors on the resident map
// (ref: src/ORBmatcher.cc:825-975, src/LocalMapping.cc:2514-2594).  orbhip_fuse_row: the points of one key
// frame's row into K target key frames; orbhip_fuse_collect: the ordered union of several rows into one.  The projection kernel
// (k_fuse.hip) writes the queries, the window search reads the targets' resident sets through one record each and the points'
// descriptors from the store by slot.  One packed upload, one dependency chain, one result block, one synchronisation; nothing is
// allocated beyond the grow-only scratch of the context.
#include "localmap_store.h"

extern "C" int orbhip_fuse_row(orbhip_ctx *c, uint64_t src_row_key, const orbhip_fuse_target *targets, int K, const uint8_t *skip,
                               const float *u_right, orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist,
                               int32_t *n_active)
{
    const char *who = "orbhip_fuse_row";
    if (!c || K < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (K == 0) return ORBHIP_OK;
    if (!targets || !best_idx || !best_dist || !n_active) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    OrbKfTable *Kf = kf_table(c);
    if (!Kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    auto it = Kf->rowOf.find(src_row_key);
    if (it == Kf->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame (orbhip_map_kf_put)");
    const int row = it->second, n = (int)Kf->entries[row].size();
    FuseTargets T;
    int rc;
    if ((rc = fuse_targets_resolve(c, who, targets, K, T))) return rc;
    if (K > FUSE_MAX_TARGETS || (int64_t)K * n > FUSE_MAX_QUERIES)
        return fail(c, ORBHIP_E_SIZE, std::string(who) + ": more than 65535 targets, or K * n beyond 2^24");
    std::vector<orbhip_local_camera> cams(K);
    if ((rc = fuse_cameras_prepare(c, targets, K, cams.data()))) return rc;
    const size_t total = (size_t)K * n;
    for (int k = 0; k < K; k++) n_active[k] = 0;
    for (size_t i = 0; i < total; i++) best_idx[i] = -1, best_dist[i] = 256;
    if (queries_out) memset(queries_out, 0, total * sizeof(orbhip_proj_query));
    if (n == 0) return ORBHIP_OK;
    HIPCHK(c, orb_enter(c));
    // scratch: the targets' feature records | the slot of every (target, entry) | the queries, unless they go back to the caller
    const size_t slotBytes = align_up(total * 4, 256), qBytes = total * sizeof(orbhip_proj_query);
    if ((rc = orb_match_scratch(c, T.recBytes + slotBytes + (queries_out ? 0 : qBytes) + 256))) return rc;
    uint8_t *scratch = c->d_match.as<uint8_t>();
    int32_t *dslots = (int32_t *)(scratch + T.recBytes);
    Packed P(c);
    const size_t tb = fuse_target_bytes();
    if ((rc = P.begin((size_t)K * (tb + sizeof(orbhip_local_camera) + 4) + (skip ? total : 0) + (u_right ? T.urTotal * 4 : 0) + total * 8 +
                      qBytes + 12 * 256)))
        return rc;
    const orbhip_local_camera *dcam = (const orbhip_local_camera *)P.in(cams.data(), (size_t)K * sizeof(orbhip_local_camera));
    const uint8_t *dskip = skip ? (const uint8_t *)P.in(skip, total) : nullptr;
    const float *dur = u_right ? (const float *)P.in(u_right, T.urTotal * 4) : nullptr;
    const void *dtab = fuse_targets_pack(P, T, scratch, targets, dur);
    int32_t *dna = (int32_t *)P.in_fill(0, (size_t)K * 4);   // the active counts (come back with what follows)
    int32_t *dbi = (int32_t *)P.out(total * 4), *dbd = (int32_t *)P.out(total * 4);
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out(qBytes) : (orbhip_proj_query *)(scratch + T.recBytes + slotBytes);
    if ((rc = P.upload())) return rc;
    launch_project_fuse_row(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints,
                            Kf->rows.as<uint8_t>() + (size_t)row * Kf->stride * 8, Kf->maxRow, dskip, dcam, n, K, dq, dslots, dna);
    launch_window_best_sets(c->stream, dtab, K, T.maxN, dq, M->desc.as<void>(), dslots, n, dbi, dbd);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dna))) return rc;   // counts | best_idx | best_dist | queries: one copy back, one synchronisation
    memcpy(n_active, P.host(dna), (size_t)K * 4);
    memcpy(best_idx, P.host(dbi), total * 4);
    memcpy(best_dist, P.host(dbd), total * 4);
    if (queries_out) memcpy(queries_out, P.host(dq), qBytes);
    return ORBHIP_OK;
}

extern "C" int orbhip_fuse_collect(orbhip_ctx *c, const orbhip_fuse_target *target, uint64_t cur_row_key, int nkf, const uint64_t *kf_keys,
                                   const float *u_right, uint64_t *keys_out, int cap, int *ncand, orbhip_proj_query *queries_out,
                                   int32_t *best_idx, int32_t *best_dist, int32_t *n_active)
{
    const char *who = "orbhip_fuse_collect";
    if (!c || !target || nkf < 0 || (nkf > 0 && !kf_keys) || cap < 0 || (cap > 0 && (!keys_out || !best_idx || !best_dist)) || !ncand ||
        !n_active)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    OrbKfTable *Kf = kf_table(c);
    if (!Kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    auto it = Kf->rowOf.find(cur_row_key);
    if (it == Kf->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame (orbhip_map_kf_put)");
    const std::vector<uint64_t> &own = Kf->entries[it->second];
    FuseTargets T;
    int rc;
    if ((rc = fuse_targets_resolve(c, who, target, 1, T))) return rc;
    std::vector<int32_t> rowIdx;
    std::vector<uint32_t> off;
    if ((rc = kf_call_rows(c, Kf, who, nkf, kf_keys, rowIdx, off))) return rc;
    orbhip_local_camera cm = target->cam;
    if ((rc = orbhip_local_camera_prepare(c, &cm))) return rc;
    KfCall Q;
    Q.total = off[nkf];
    *ncand = 0;
    *n_active = 0;
    if (Q.total == 0) return ORBHIP_OK;
    const int capQ = (int)std::min<uint64_t>(Q.total, (uint64_t)cap);
    if (capQ == 0) {   // nothing can be returned: the count alone
        uint64_t none;
        return orbhip_map_collect(c, nkf, kf_keys, &none, 0, ncand);
    }
    HIPCHK(c, orb_enter(c));
    if ((rc = kf_call_scratch(c, Kf, Q, capQ))) return rc;
    const OrbSetView &S = T.view[0];
    const size_t qBytes = (size_t)capQ * sizeof(orbhip_proj_query), slotBytes = align_up((size_t)capQ * 4, 256);
    if ((rc = orb_match_scratch(c, T.recBytes + slotBytes + (queries_out ? 0 : qBytes) + 256))) return rc;
    uint8_t *scratch = c->d_match.as<uint8_t>();
    int32_t *dqslot = (int32_t *)(scratch + T.recBytes);
    Packed P(c);
    const size_t tb = fuse_target_bytes();
    if ((rc = P.begin(tb + sizeof cm + (size_t)nkf * 8 + 4 + own.size() * 4 + (u_right ? (size_t)S.n * 4 : 0) + (size_t)capQ * 12 + qBytes +
                      14 * 256)))
        return rc;
    const orbhip_local_camera *dcam = (const orbhip_local_camera *)P.in(&cm, sizeof cm);
    Q.d_rowIdx = (const int32_t *)P.in(rowIdx.data(), (size_t)nkf * 4);
    Q.d_off = (const uint32_t *)P.in(off.data(), (size_t)(nkf + 1) * 4);
    // IsInKeyFrame(pKF): the slots the current key frame's row resolves to on the host's mirror (the entry's generation is the
    // slot's); a bad point among them is marked too, and is no candidate anyway
    int32_t *hown;
    const int32_t *down = (const int32_t *)P.in_reserve(own.size() * 4, (void **)&hown);
    for (size_t i = 0; i < own.size(); i++) {
        const int32_t s = own[i] == ~(uint64_t)0 ? -1 : (int32_t)(uint32_t)own[i];
        hown[i] = (s >= 0 && s < M->maxPoints && M->slotKey[s] != 0 && M->gen[s] == (uint32_t)(own[i] >> 32)) ? s : -1;
    }
    const float *dur = u_right ? (const float *)P.in(u_right, (size_t)S.n * 4) : nullptr;
    const void *dtab = fuse_targets_pack(P, T, scratch, target, dur);
    const int32_t cnts[4] = {0, 0, 0, 0};
    int32_t *dc = (int32_t *)P.in(cnts, 16);   // candidates | active queries (come back with what follows)
    int32_t *dslots = (int32_t *)P.out((size_t)capQ * 4);
    int32_t *dbi = (int32_t *)P.out((size_t)capQ * 4), *dbd = (int32_t *)P.out((size_t)capQ * 4);
    orbhip_proj_query *dq = queries_out ? (orbhip_proj_query *)P.out(qBytes) : (orbhip_proj_query *)(scratch + T.recBytes + slotBytes);
    if ((rc = P.upload())) return rc;
    uint32_t *marks = Kf->marks.as<uint32_t>();
    launch_collect(c->stream, Kf->rows.as<void>(), Kf->rowHigh, Kf->stride, Q.d_rowIdx, Q.d_off, nkf, Q.total, M->flags.as<uint32_t>(),
                   M->maxPoints, marks, Kf->first.as<uint32_t>(), Q.d_cand, Q.d_blockCnt, capQ, dslots, nullptr, dc);
    launch_mark_add(c->stream, down, (int)own.size(), M->maxPoints, marks);
    launch_project_fuse_list(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints, marks, dslots, dc,
                             dcam, capQ, dq, dqslot, dc + 1);
    launch_mark_clear(c->stream, down, (int)own.size(), M->maxPoints, marks);
    launch_window_best_sets(c->stream, dtab, 1, S.n, dq, M->desc.as<void>(), dqslot, capQ, dbi, dbd);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dc))) return rc;   // counts | slots | best_idx | best_dist | queries: one copy back, one synchronisation
    const int32_t *hc = (const int32_t *)P.host(dc);
    const int got = hc[0];
    *ncand = got;
    if ((rc = collect_keys_out(c, M, (const int32_t *)P.host(dslots), got, capQ, cap, keys_out,
                               std::string(who) + ": more candidates than cap (*ncand has the number)")))
        return rc;
    *n_active = hc[1];
    memcpy(best_idx, P.host(dbi), (size_t)got * 4);
    memcpy(best_dist, P.host(dbd), (size_t)got * 4);
    if (queries_out) memcpy(queries_out, P.host(dq), (size_t)got * sizeof(orbhip_proj_query));
    return ORBHIP_OK;
}
