// api_correct.hip -- C ABI, part 17: map points moved in place on the resident store.
// orbhip_map_correct_sim3: the point loop of LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-568) -- the position through two
// Sim3 maps in double, then MapPoint::UpdateNormalAndDepth with the camera centres the observers have at the point's turn of the
// reference's sequence.  orbhip_map_correct_se3: the point loop of LoopClosing::RunGlobalBundleAdjustment (ref: :762-797).  Kernels
// in k_correct.hip.  Every argument is checked before any device work: a failed call changes nothing.  One packed upload, one launch,
// one result block, one synchronisation.
#include "localmap_store.h"

#define CORRECT_MAX_LIST (1 << 20)   // rows of one list, as orbhip_map_refresh

// the slots of P distinct keys of the store
static int correct_slots(orbhip_ctx *c, OrbLocalMap *M, const char *who, int P, const uint64_t *point_keys, std::vector<int32_t> &slots)
{
    slots.resize(P);
    {
        std::vector<uint64_t> k(point_keys, point_keys + P);
        std::sort(k.begin(), k.end());
        if (std::adjacent_find(k.begin(), k.end()) != k.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a point key appears twice");
    }
    for (int p = 0; p < P; p++) {
        auto it = point_keys[p] ? M->slotOf.find(point_keys[p]) : M->slotOf.end();
        if (it == M->slotOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a point key is not in the store");
        slots[p] = it->second;
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_map_correct_sim3(orbhip_ctx *c, const orbhip_refresh_params *prm, int K, const orbhip_correct_xf *xf, int nkf,
                                       const orbhip_correct_kf *kfs, int P, const uint64_t *point_keys, const int32_t *corr,
                                       const int32_t *off, const int32_t *obs_kf, const int32_t *ref_pos, const uint8_t *ref_level,
                                       uint8_t *status, float *pos_out, float *normal_out, float *min_dist_out, float *max_dist_out)
{
    const char *who = "orbhip_map_correct_sim3";
    if (!c || !prm || nkf < 0 || P < 0 || K < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    if (P == 0) return ORBHIP_OK;
    if (K < 1) return fail(c, ORBHIP_E_ARG, std::string(who) + ": points, but no corrected key frame");
    if (!xf || !point_keys || !corr || !off || !ref_pos || !ref_level || !status || (nkf > 0 && !kfs))
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (prm->nlevels < 1 || prm->nlevels > ORBHIP_MAX_LEVELS) return fail(c, ORBHIP_E_ARG, std::string(who) + ": nlevels outside 1..16");
    if (off[0] != 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": off[0] must be 0");
    for (int p = 0; p < P; p++)
        if (off[p + 1] < off[p]) return fail(c, ORBHIP_E_ARG, std::string(who) + ": offsets must ascend");
    for (int p = 0; p < P; p++)
        if (off[p + 1] - off[p] >= CORRECT_MAX_LIST) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": a list of 2^20 rows or more");
    const int total = off[P];
    if (total > 0 && !obs_kf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    std::vector<int32_t> slots;
    int rc;
    if ((rc = correct_slots(c, M, who, P, point_keys, slots))) return rc;
    {
        std::vector<uint8_t> taken(K, 0);
        for (int i = 0; i < nkf; i++) {
            const int r = kfs[i].rank;
            if (r < -1 || r >= K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a rank outside [-1, K)");
            if (r >= 0 && taken[r]++) return fail(c, ORBHIP_E_ARG, std::string(who) + ": two key frames of one rank");
        }
    }
    for (int j = 0; j < total; j++)
        if (obs_kf[j] < 0 || obs_kf[j] >= nkf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": obs_kf outside the key frames of the call");
    for (int p = 0; p < P; p++) {
        const int N = off[p + 1] - off[p];
        if (corr[p] < 0 || corr[p] >= K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": corr outside [0, K)");
        if (N > 0 && (ref_pos[p] < 0 || ref_pos[p] >= N)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": ref_pos outside the point's list");
        if (ref_level[p] >= prm->nlevels) return fail(c, ORBHIP_E_ARG, std::string(who) + ": ref_level outside [0, nlevels)");
    }

    HIPCHK(c, orb_enter(c));
    Packed Pk(c);
    const size_t nP = (size_t)P;
    if ((rc = Pk.begin((size_t)K * sizeof *xf + (size_t)nkf * sizeof *kfs + sizeof *prm + nP * 17 + 4 + (size_t)total * 4 + nP * (1 + 16 + 16) + 12 * 256)))
        return rc;
    const orbhip_correct_xf *dxf = (const orbhip_correct_xf *)Pk.in(xf, (size_t)K * sizeof *xf);
    const orbhip_correct_kf *dkf = (const orbhip_correct_kf *)Pk.in(kfs, (size_t)nkf * sizeof *kfs);
    const orbhip_refresh_params *dprm = (const orbhip_refresh_params *)Pk.in(prm, sizeof *prm);
    const int32_t *dslots = (const int32_t *)Pk.in(slots.data(), nP * 4);
    const int32_t *dcorr = (const int32_t *)Pk.in(corr, nP * 4);
    const int32_t *doff = (const int32_t *)Pk.in(off, (nP + 1) * 4);
    const int32_t *dref = (const int32_t *)Pk.in(ref_pos, nP * 4);
    const uint8_t *dlev = (const uint8_t *)Pk.in(ref_level, nP);
    const int32_t *dobs = (const int32_t *)Pk.in(obs_kf, (size_t)total * 4);
    uint8_t *dst = (uint8_t *)Pk.out(nP);
    void *dA = Pk.out(nP * 16), *dB = Pk.out(nP * 16);
    if ((rc = Pk.upload())) return rc;
    launch_map_correct_sim3(c->stream, dxf, dkf, dprm, dslots, dcorr, doff, dobs, dref, dlev, P, K, M->maxPoints, M->geoA.as<void>(),
                            M->geoB.as<void>(), M->flags.as<uint32_t>(), dst, dA, dB);
    HIPCHK(c, hipGetLastError());
    if ((rc = Pk.download())) return rc;   // status | position, min | normal, max: one copy back, one synchronisation
    memcpy(status, Pk.host(dst), nP);
    const float *hA = (const float *)Pk.host(dA), *hB = (const float *)Pk.host(dB);
    for (size_t p = 0; p < nP; p++) {
        if (pos_out) pos_out[3 * p] = hA[4 * p], pos_out[3 * p + 1] = hA[4 * p + 1], pos_out[3 * p + 2] = hA[4 * p + 2];
        if (min_dist_out) min_dist_out[p] = hA[4 * p + 3];
        if (normal_out) normal_out[3 * p] = hB[4 * p], normal_out[3 * p + 1] = hB[4 * p + 1], normal_out[3 * p + 2] = hB[4 * p + 2];
        if (max_dist_out) max_dist_out[p] = hB[4 * p + 3];
    }
    return ORBHIP_OK;
}

extern "C" int orbhip_map_correct_se3(orbhip_ctx *c, int K, const orbhip_correct_se3 *xf, int P, const uint64_t *point_keys,
                                      const int32_t *corr, const float *pos_set, uint8_t *status, float *pos_out)
{
    const char *who = "orbhip_map_correct_se3";
    if (!c || P < 0 || K < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    if (P == 0) return ORBHIP_OK;
    if (!point_keys || !corr || !status || (K > 0 && !xf)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    bool given = false;
    for (int p = 0; p < P; p++) {
        if (corr[p] < -1 || corr[p] >= K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": corr outside [-1, K)");
        given |= corr[p] == -1;
    }
    if (given && !pos_set) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a corr of -1 without pos_set");
    std::vector<int32_t> slots;
    int rc;
    if ((rc = correct_slots(c, M, who, P, point_keys, slots))) return rc;

    HIPCHK(c, orb_enter(c));
    Packed Pk(c);
    const size_t nP = (size_t)P;
    if ((rc = Pk.begin((size_t)K * sizeof *xf + nP * (4 + 4 + 12 + 1 + 12) + 8 * 256))) return rc;
    const orbhip_correct_se3 *dxf = (const orbhip_correct_se3 *)Pk.in(xf, (size_t)K * sizeof *xf);
    const int32_t *dslots = (const int32_t *)Pk.in(slots.data(), nP * 4);
    const int32_t *dcorr = (const int32_t *)Pk.in(corr, nP * 4);
    const float *dset = given ? (const float *)Pk.in(pos_set, nP * 12) : nullptr;
    uint8_t *dst = (uint8_t *)Pk.out(nP);
    float *dpos = (float *)Pk.out(nP * 12);
    if ((rc = Pk.upload())) return rc;
    launch_map_correct_se3(c->stream, dxf, dslots, dcorr, dset, P, K, M->maxPoints, M->geoA.as<void>(), M->flags.as<uint32_t>(), dst, dpos);
    HIPCHK(c, hipGetLastError());
    if ((rc = Pk.download())) return rc;
    memcpy(status, Pk.host(dst), nP);
    if (pos_out) memcpy(pos_out, Pk.host(dpos), nP * 12);
    return ORBHIP_OK;
}
