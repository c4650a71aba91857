// api_bowcand.hip -- C ABI, part 15: SearchByBoW against all candidate key frames in one call.
// orbhip_search_by_bow_candidates: Tracking::Relocalization (ref: src/Tracking.cc:2595-2616) and LoopClosing::ComputeSim3 (ref:
// src/LoopClosing.cc:304-332) call ORBmatcher::SearchByBoW once per candidate key frame.  Here every key frame is a resident set
// (api_sets.hip), "has a map point that is not bad" is what its row of the key-frame table answers (api_localmap.hip), and the
// rotation check and -- for relocalisation -- the PnPsolver constructor's gather run on the device behind the matching
// (k_bowcand.hip).  Every argument is checked before any device work; one packed upload (pair records, candidate records, the
// per-level table), the kernels enqueued back to back, one result block in page-locked memory, one synchronisation.
#include "localmap_store.h"

extern "C" int orbhip_search_by_bow_candidates(orbhip_ctx *c, int mode, uint64_t fixed_set_key, uint64_t fixed_row_key,
                                               const orbhip_bow_candidate *cand, int K, int th, float nnratio, int check_ori,
                                               int32_t *matches, int32_t *nmatches, int min_matches, const float *level_sigma2,
                                               int nlevels, float th2, int32_t *off, int32_t *kp_idx, int32_t *kf_idx, float *P3Dw,
                                               float *P2D, float *max_err, int cap, int *ntotal)
{
    const std::string who = "orbhip_search_by_bow_candidates";
    if (!c || K < 0 || (mode != 0 && mode != 1)) return fail(c, ORBHIP_E_ARG, who + ": bad argument");
    if (K == 0) return ORBHIP_OK;
    if (!cand || !matches || !nmatches) return fail(c, ORBHIP_E_ARG, who + ": bad argument");
    if (K > BOW_CAND_MAX_K) return fail(c, ORBHIP_E_ARG, who + ": more than 4095 candidates in one call");
    const bool anyGather = level_sigma2 || off || kp_idx || kf_idx || P3Dw || P2D || max_err || ntotal;
    const bool gather = level_sigma2 && off && kp_idx && kf_idx && P3Dw && P2D && max_err && ntotal;
    if (anyGather && (!gather || mode != 0 || cap < 0 || nlevels < 1 || nlevels > 64))
        return fail(c, ORBHIP_E_ARG, who + ": the gather outputs are for mode 0, all of them or none; nlevels within 1..64, cap >= 0");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *T = kf_table(c);
    if (!M || !T) return fail(c, ORBHIP_E_ARG, who + ": no store or no key-frame table (orbhip_map_init, orbhip_map_kf_init)");
    {
        std::vector<uint64_t> keys(1, fixed_set_key);
        for (int k = 0; k < K; k++)
            if (std::find(keys.begin(), keys.end(), cand[k].set_key) == keys.end()) keys.push_back(cand[k].set_key);
        if ((int)keys.size() > orb_set_limit_in_force(c))
            return fail(c, ORBHIP_E_ARG, who + ": more distinct sets than the set limit in force (orbhip_set_limit)");
    }
    OrbSetBow F = {};
    if (!orb_set_bow_view(c, fixed_set_key, &F)) return fail(c, ORBHIP_E_ARG, who + ": the fixed side is an unknown set (orbhip_set_put)");
    const int nF = F.n;
    int rowF = -1;
    if (mode == 1) {
        auto it = T->rowOf.find(fixed_row_key);
        if (it == T->rowOf.end()) return fail(c, ORBHIP_E_ARG, who + ": the fixed side is an unknown key frame (orbhip_map_kf_put)");
        rowF = it->second;
        if ((int)T->entries[rowF].size() != nF) return fail(c, ORBHIP_E_ARG, who + ": the fixed key frame's row and its set differ in length");
    }
    std::vector<OrbSetBow> S(K);
    std::vector<int32_t> rowC(K);
    size_t totalC = 0;
    for (int k = 0; k < K; k++) {
        if (!orb_set_bow_view(c, cand[k].set_key, &S[k])) return fail(c, ORBHIP_E_ARG, who + ": a candidate is an unknown set (orbhip_set_put)");
        auto it = T->rowOf.find(cand[k].row_key);
        if (it == T->rowOf.end()) return fail(c, ORBHIP_E_ARG, who + ": a candidate is an unknown key frame (orbhip_map_kf_put)");
        rowC[k] = it->second;
        if ((int)T->entries[rowC[k]].size() != S[k].n)
            return fail(c, ORBHIP_E_ARG, who + ": a candidate's row and its set differ in length");
        totalC += (size_t)S[k].n;
    }
    // (bow_match_node keeps the position inside a node's side-2 list in 20 bits; the pair record keeps a candidate's node in 20)
    auto entries = [](const OrbSetBow &s) { return s.ng > 0 ? s.off[s.ng] : 0; };
    if (mode == 0 && entries(F) >= (1 << 20)) return fail(c, ORBHIP_E_SIZE, who + ": more than 2^20 - 1 entries in the second FeatureVector");
    for (int k = 0; k < K; k++)
        if ((mode == 1 && entries(S[k]) >= (1 << 20)) || S[k].ng >= (1 << BOW_CAND_NODE_BITS))
            return fail(c, ORBHIP_E_SIZE, who + ": more than 2^20 - 1 entries in the second FeatureVector");
    if (totalC > (size_t)INT32_MAX || (size_t)K * (size_t)nF > (size_t)INT32_MAX)
        return fail(c, ORBHIP_E_SIZE, who + ": K * n_fixed or the candidates' features above 2^31 - 1");
    if (gather && (F.octMin < 0 || F.octMax >= nlevels)) return fail(c, ORBHIP_E_ARG, who + ": the frame's set has an octave outside [0, nlevels)");

    std::vector<BowCandPair> pairs;
    std::vector<BowCandDev> tab(K);
    const uint8_t *rows = T->rows.as<uint8_t>();
    const size_t rowBytes = (size_t)T->stride * 8;
    size_t at = 0;
    for (int k = 0; k < K; k++) {
        const OrbSetBow &s = S[k];
        tab[k] = {s.d_desc, s.d_off, s.d_idx, s.d_kps, rows + (size_t)rowC[k] * rowBytes, s.n, (int)at, k, 0};
        at += (size_t)s.n;
        for (int gF = 0, gC = 0; gF < F.ng && gC < s.ng;) {     // merge walk over the two FeatureVectors (ref: :180-264, :550-632)
            if (F.node[gF] == s.node[gC]) {
                if (F.off[gF + 1] > F.off[gF] && s.off[gC + 1] > s.off[gC])
                    pairs.push_back({(uint32_t)gF, ((uint32_t)k << BOW_CAND_NODE_BITS) | (uint32_t)gC});
                gF++;
                gC++;
            } else if (F.node[gF] < s.node[gC])
                gF++;
            else
                gC++;
        }
    }
    const int npairs = (int)pairs.size();
    const size_t rowsBytes = (size_t)K * nF * 4;
    if (npairs == 0) {   // no candidate shares a node with the fixed side: nothing for the device to do
        if (gather) {
            *ntotal = 0;
            for (int k = 0; k <= K; k++) off[k] = 0;
        }
        memset(matches, 0xFF, rowsBytes);
        for (int k = 0; k < K; k++) nmatches[k] = 0;
        return ORBHIP_OK;
    }
    HIPCHK(c, orb_enter(c));
    const int capDev = gather ? (int)std::min<size_t>((size_t)cap, (size_t)K * nF) : 0;
    Packed P(c);
    int rc;
    if ((rc = P.begin(pairs.size() * sizeof(BowCandPair) + tab.size() * sizeof(BowCandDev) + (size_t)nlevels * 4 + 2 * rowsBytes +
                      totalC * 4 + (size_t)K * 12 + 64 + (size_t)capDev * 32 + 24 * 256)))
        return rc;
    const BowCandPair *dp = (const BowCandPair *)P.in(pairs.data(), pairs.size() * sizeof(BowCandPair));
    const BowCandDev *dt = (const BowCandDev *)P.in(tab.data(), tab.size() * sizeof(BowCandDev));
    const float *dsg = gather ? (const float *)P.in(level_sigma2, (size_t)nlevels * 4) : nullptr;
    // out rows | reverse arrays: adjacent on the device, -1 by one device memset; the per-candidate counts for the gather's scan
    int32_t *dout = (int32_t *)P.out(align_up(rowsBytes, 256) + totalC * 4);
    int32_t *dscr = (int32_t *)((uint8_t *)dout + align_up(rowsBytes, 256));
    int32_t *dnm = (int32_t *)P.out((size_t)K * 4);
    // the result block: written by plain stores over PCIe, no copy back
    int32_t *hrows = (int32_t *)P.out_host(rowsBytes), *hnm = (int32_t *)P.out_host((size_t)K * 4);
    int32_t *hoff = nullptr, *hnt = nullptr, *hkp = nullptr, *hkf = nullptr;
    float *hP3 = nullptr, *hP2 = nullptr, *hme = nullptr;
    if (gather) {
        hoff = (int32_t *)P.out_host((size_t)(K + 1) * 4);
        hnt = (int32_t *)P.out_host(16);
        hkp = (int32_t *)P.out_host((size_t)capDev * 4);
        hkf = (int32_t *)P.out_host((size_t)capDev * 4);
        hP3 = (float *)P.out_host((size_t)capDev * 12);
        hP2 = (float *)P.out_host((size_t)capDev * 8);
        hme = (float *)P.out_host((size_t)capDev * 4);
    }
    if ((rc = P.upload())) return rc;
    HIPCHK(c, hipMemsetAsync(dout, 0xFF, align_up(rowsBytes, 256) + totalC * 4, c->stream));
    const uint32_t *mflags = M->flags.as<uint32_t>();
    launch_bow_match_cands(c->stream, mode, F.d_desc, F.d_off, F.d_idx, rowF >= 0 ? rows + (size_t)rowF * rowBytes : nullptr, nF, dt, dp,
                           npairs, mflags, M->maxPoints, th, nnratio, dout, dscr);
    launch_bow_rot_cands(c->stream, mode, dt, K, F.d_kps, nF, check_ori ? 1 : 0, dout, hrows, dnm, hnm);
    if (gather)
        launch_pnp_gather_cands(c->stream, dt, K, dnm, min_matches, F.d_kps, nF, dout, dsg, nlevels, th2, M->geoA.as<void>(), mflags,
                                M->maxPoints, capDev, hoff, hnt, hkp, hkf, hP3, hP2, hme);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (gather) {
        const int total = *hnt;
        if (total < 0 || (size_t)total > (size_t)K * nF) return fail(c, ORBHIP_E_HIP, who + ": internal: correspondence count out of range");
        if (total > cap) {
            *ntotal = total;
            return fail(c, ORBHIP_E_CAPACITY, who + ": more correspondences than cap (*ntotal has the number)");
        }
        *ntotal = total;
        memcpy(off, hoff, (size_t)(K + 1) * 4);
        memcpy(kp_idx, hkp, (size_t)total * 4);
        memcpy(kf_idx, hkf, (size_t)total * 4);
        memcpy(P3Dw, hP3, (size_t)total * 12);
        memcpy(P2D, hP2, (size_t)total * 8);
        memcpy(max_err, hme, (size_t)total * 4);
    }
    memcpy(matches, hrows, rowsBytes);
    memcpy(nmatches, hnm, (size_t)K * 4);
    return ORBHIP_OK;
}
