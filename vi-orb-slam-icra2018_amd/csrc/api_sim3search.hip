// api_sim3search.hip -- C ABI, part 19: ORBmatcher::SearchBySim3 on the resident map (ref: src/ORBmatcher.cc:1102-1326, called by
// LoopClosing::ComputeSim3 at src/LoopClosing.cc:375).  orbhip_search_by_sim3: the points of both key
// frames' rows projected into the other key frame through the similarity between the cameras (k_project_sim3), searched in the
// other key frame's resident set (k_window_best_sets of k_fuse.hip with two target records, chi-square gate off, the descriptor
// read from the store by slot) and the two tables turned into the mutual matches (k_sim3_agree).  One packed upload -- the two
// camera records, the similarity, the taken bytes --, one dependency chain, one result block, one synchronisation; nothing is
// allocated beyond the grow-only scratch of the context.
#include "localmap_store.h"

extern "C" int orbhip_search_by_sim3(orbhip_ctx *c, const orbhip_fuse_target *sides, const uint64_t *row_keys, const float *sR21,
                                     const float *t21, const float *sR12, const float *t12, float th, int th_high, const uint8_t *taken1,
                                     const uint8_t *taken2, int32_t *match12, int *nfound, int32_t *n_active,
                                     orbhip_proj_query *queries1_out, int32_t *best1, int32_t *dist1, orbhip_proj_query *queries2_out,
                                     int32_t *best2, int32_t *dist2)
{
    const char *who = "orbhip_search_by_sim3";
    if (!c || !sides || !row_keys || !sR21 || !t21 || !sR12 || !t12 || !match12 || !nfound || !n_active)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (!std::isfinite(th)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": th not finite");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    OrbKfTable *Kf = kf_table(c);
    if (!Kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    int row[2];
    for (int s = 0; s < 2; s++) {
        auto it = Kf->rowOf.find(row_keys[s]);
        if (it == Kf->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame (orbhip_map_kf_put)");
        row[s] = it->second;
    }
    // the search of direction d runs in the OTHER side's set: target record d is side 1 - d
    orbhip_fuse_target dst[2] = {sides[1], sides[0]};
    dst[0].cam.th = dst[1].cam.th = th;
    FuseTargets T;
    int rc;
    if ((rc = fuse_targets_resolve(c, who, dst, 2, T))) return rc;
    const int n1 = T.view[1].n, n2 = T.view[0].n;
    if ((int)Kf->entries[row[0]].size() != n1 || (int)Kf->entries[row[1]].size() != n2)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": a row is not as long as its set has features (the matches index both)");
    const int capQ = std::max(n1, n2);
    if ((int64_t)2 * capQ > FUSE_MAX_QUERIES) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": 2 * n beyond 2^24");
    orbhip_local_camera cams[2];
    if ((rc = fuse_cameras_prepare(c, sides, 2, cams))) return rc;
    cams[0].th = cams[1].th = th;
    // every check has passed: the outputs as two rows without a point leave them
    *nfound = 0;
    n_active[0] = n_active[1] = 0;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    bool any = false;
    for (int s = 0; s < 2 && !any; s++)
        for (uint64_t e : Kf->entries[row[s]])
            if (e != ~(uint64_t)0) {
                any = true;
                break;
            }
    if (!any) {   // two rows without a point: nothing is launched
        if (queries1_out) memset(queries1_out, 0, (size_t)n1 * sizeof(orbhip_proj_query));
        if (queries2_out) memset(queries2_out, 0, (size_t)n2 * sizeof(orbhip_proj_query));
        for (int i = 0; i < n1; i++) {
            if (best1) best1[i] = -1;
            if (dist1) dist1[i] = 256;
        }
        for (int i = 0; i < n2; i++) {
            if (best2) best2[i] = -1;
            if (dist2) dist2[i] = 256;
        }
        return ORBHIP_OK;
    }
    HIPCHK(c, orb_enter(c));
    // scratch: the two sets' feature records | the slot of every (direction, entry) | the two tables and the queries, unless they
    // go back to the caller
    const bool wantQ = queries1_out || queries2_out, wantB = best1 || dist1 || best2 || dist2;
    const size_t total = (size_t)2 * capQ;
    const size_t slotBytes = align_up(total * 4, 256), tabBytes = align_up(total * 4, 256), qBytes = total * sizeof(orbhip_proj_query);
    if ((rc = orb_match_scratch(c, T.recBytes + slotBytes + (wantB ? 0 : 2 * tabBytes) + (wantQ ? 0 : qBytes) + 256))) return rc;
    uint8_t *scratch = c->d_match.as<uint8_t>();
    int32_t *dqslot = (int32_t *)(scratch + T.recBytes);
    uint8_t *spare = scratch + T.recBytes + slotBytes;
    Packed P(c);
    const size_t tb = fuse_target_bytes();
    if ((rc = P.begin(2 * tb + sizeof cams + sim3_pair_bytes() + (size_t)n1 + (size_t)n2 + 16 + (size_t)n1 * 4 + 2 * tabBytes + qBytes + 12 * 256)))
        return rc;
    const orbhip_local_camera *dcam = (const orbhip_local_camera *)P.in(cams, sizeof cams);
    void *hpair;
    const void *dpair = P.in_reserve(sim3_pair_bytes(), &hpair);
    sim3_pair_fill(hpair, sR21, t21, sR12, t12, row[0], row[1], n1, n2, th, th_high);
    const uint8_t *dtk1 = taken1 ? (const uint8_t *)P.in(taken1, (size_t)n1) : nullptr;
    const uint8_t *dtk2 = taken2 ? (const uint8_t *)P.in(taken2, (size_t)n2) : nullptr;
    const void *dtab = fuse_targets_pack(P, T, scratch, dst, nullptr);
    int32_t *dc = (int32_t *)P.in_fill(0, 16);   // active queries of the two directions | matches (come back with what follows)
    int32_t *dm = (int32_t *)P.out((size_t)n1 * 4);
    int32_t *dbi = wantB ? (int32_t *)P.out(total * 4) : (int32_t *)spare;
    int32_t *dbd = wantB ? (int32_t *)P.out(total * 4) : (int32_t *)(spare + tabBytes);
    orbhip_proj_query *dq = wantQ ? (orbhip_proj_query *)P.out(qBytes) : (orbhip_proj_query *)(spare + (wantB ? 0 : 2 * tabBytes));
    if ((rc = P.upload())) return rc;
    launch_project_sim3(c->stream, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->maxPoints, Kf->rows.as<void>(),
                        Kf->stride, Kf->maxRow, dpair, dcam, dtk1, dtk2, capQ, dq, dqslot, dc);
    launch_window_best_sets(c->stream, dtab, 2, T.maxN, dq, M->desc.as<void>(), dqslot, capQ, dbi, dbd, /*gate*/ false);
    launch_sim3_agree(c->stream, dpair, dbi, dbd, capQ, n1, dm, dc + 2);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dc))) return rc;   // counts | match12 | the tables | the queries: one copy back, one synchronisation
    const int32_t *hc = (const int32_t *)P.host(dc);
    n_active[0] = hc[0], n_active[1] = hc[1];
    *nfound = hc[2];
    memcpy(match12, P.host(dm), (size_t)n1 * 4);
    if (wantB) {
        const int32_t *hbi = (const int32_t *)P.host(dbi), *hbd = (const int32_t *)P.host(dbd);
        if (best1) memcpy(best1, hbi, (size_t)n1 * 4);
        if (dist1) memcpy(dist1, hbd, (size_t)n1 * 4);
        if (best2) memcpy(best2, hbi + capQ, (size_t)n2 * 4);
        if (dist2) memcpy(dist2, hbd + capQ, (size_t)n2 * 4);
    }
    if (wantQ) {
        const orbhip_proj_query *hq = (const orbhip_proj_query *)P.host(dq);
        if (queries1_out) memcpy(queries1_out, hq, (size_t)n1 * sizeof(orbhip_proj_query));
        if (queries2_out) memcpy(queries2_out, hq + capQ, (size_t)n2 * sizeof(orbhip_proj_query));
    }
    return ORBHIP_OK;
}
