// api_refresh.hip -- C ABI, part 13: map points refreshed in place on the resident store.
// orbhip_map_refresh: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (ref: src/MapPoint.cc:257-322,
// :345-386) for a batch of points from their observation lists -- the observers' descriptors and octaves come from the resident
// feature sets, the position from the store (k_refresh.hip).  orbhip_map_get: read-back of store entries.  Every argument is
// checked before any device work: a failed call changes nothing.  One packed upload, one launch, one result block, one
// synchronisation.
#include "localmap_store.h"

#define REFRESH_MAX_LIST (1 << 20)   // rows of one list: the kernel keeps a position in 20 bits

extern "C" int orbhip_map_refresh(orbhip_ctx *c, const orbhip_refresh_params *prm, int nkf, const orbhip_refresh_kf *kfs, int P,
                                  const uint64_t *point_keys, const int32_t *off, const int32_t *obs_kf, const int32_t *obs_idx,
                                  const int32_t *ref_pos, uint8_t *status, int32_t *best_pos, uint8_t *desc_out, float *normal_out,
                                  float *min_dist_out, float *max_dist_out)
{
    const char *who = "orbhip_map_refresh";
    if (!c || !prm || nkf < 0 || P < 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    if (P == 0) return ORBHIP_OK;
    const bool wantNormal = (prm->what & ORBHIP_REFRESH_NORMAL) != 0;
    if (!point_keys || !off || !status || (nkf > 0 && !kfs) || (wantNormal && !ref_pos))
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (prm->what < 1 || prm->what > (ORBHIP_REFRESH_DESC | ORBHIP_REFRESH_NORMAL))
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": what is neither ORBHIP_REFRESH_DESC, ORBHIP_REFRESH_NORMAL nor both");
    if (prm->nlevels < 1 || prm->nlevels > ORBHIP_MAX_LEVELS) return fail(c, ORBHIP_E_ARG, std::string(who) + ": nlevels outside 1..16");
    if (off[0] != 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": off[0] must be 0");
    for (int p = 0; p < P; p++)
        if (off[p + 1] < off[p]) return fail(c, ORBHIP_E_ARG, std::string(who) + ": offsets must ascend");
    for (int p = 0; p < P; p++)
        if (off[p + 1] - off[p] >= REFRESH_MAX_LIST) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": a list of 2^20 rows or more");
    const int total = off[P];
    if (total > 0 && (!obs_kf || !obs_idx)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    // the points
    std::vector<int32_t> slots(P);
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
    // the key frames
    {
        std::vector<uint64_t> k;
        for (int i = 0; i < nkf; i++) k.push_back(kfs[i].set_key);
        std::sort(k.begin(), k.end());
        if ((int)(std::unique(k.begin(), k.end()) - k.begin()) > orb_set_limit_in_force(c))
            return fail(c, ORBHIP_E_ARG, std::string(who) + ": more distinct sets than the set limit in force (orbhip_set_limit)");
    }
    std::vector<OrbSetKps> view(nkf);
    for (int i = 0; i < nkf; i++) {
        if (!orb_set_kps_view(c, kfs[i].set_key, &view[i])) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a set is not resident (orbhip_set_put)");
        if (view[i].n > 0 && (view[i].octMin < 0 || view[i].octMax >= prm->nlevels))
            return fail(c, ORBHIP_E_ARG, std::string(who) + ": a set has an octave outside [0, nlevels)");
    }
    // the lists
    for (int j = 0; j < total; j++) {
        if (obs_kf[j] < 0 || obs_kf[j] >= nkf) return fail(c, ORBHIP_E_ARG, std::string(who) + ": obs_kf outside the key frames of the call");
        if (obs_idx[j] < 0 || obs_idx[j] >= view[obs_kf[j]].n) return fail(c, ORBHIP_E_ARG, std::string(who) + ": obs_idx outside the set");
    }
    if (wantNormal)
        for (int p = 0; p < P; p++) {
            const int N = off[p + 1] - off[p];
            if (N > 0 && (ref_pos[p] < 0 || ref_pos[p] >= N)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": ref_pos outside the point's list");
        }

    HIPCHK(c, orb_enter(c));
    Packed Pk(c);
    int rc;
    const size_t nP = (size_t)P;
    if ((rc = Pk.begin((size_t)nkf * sizeof(RefreshKfDev) + sizeof *prm + nP * 12 + 4 + (size_t)total * 8 + nP * (1 + 4 + 32 + 16 + 4) + 14 * 256)))
        return rc;
    RefreshKfDev *hk;
    const RefreshKfDev *dk = (const RefreshKfDev *)Pk.in_reserve((size_t)nkf * sizeof(RefreshKfDev), (void **)&hk);
    for (int i = 0; i < nkf; i++) {
        hk[i].desc = reinterpret_cast<const uint4 *>(view[i].d_desc);
        hk[i].kps = view[i].d_kps;
        hk[i].ox = kfs[i].Ow[0], hk[i].oy = kfs[i].Ow[1], hk[i].oz = kfs[i].Ow[2];
        hk[i].flags = kfs[i].flags;
    }
    const orbhip_refresh_params *dprm = (const orbhip_refresh_params *)Pk.in(prm, sizeof *prm);
    const int32_t *dslots = (const int32_t *)Pk.in(slots.data(), nP * 4);
    const int32_t *doff = (const int32_t *)Pk.in(off, (nP + 1) * 4);
    const int32_t *dref = wantNormal ? (const int32_t *)Pk.in(ref_pos, nP * 4) : nullptr;
    int32_t *hobs;
    const void *dobs = Pk.in_reserve((size_t)total * 8, (void **)&hobs);
    for (int j = 0; j < total; j++) hobs[2 * j] = obs_kf[j], hobs[2 * j + 1] = obs_idx[j];
    uint8_t *dst = (uint8_t *)Pk.out(nP);
    int32_t *dbest = (int32_t *)Pk.out(nP * 4);
    void *ddesc = Pk.out(nP * 32);
    void *dB = Pk.out(nP * 16);
    float *dmin = (float *)Pk.out(nP * 4);
    if ((rc = Pk.upload())) return rc;
    launch_map_refresh(c->stream, dk, dprm, dslots, doff, dobs, dref, P, M->maxPoints, M->geoA.as<void>(), M->geoB.as<void>(),
                       M->flags.as<uint32_t>(), M->desc.as<void>(), dst, dbest, ddesc, dB, dmin);
    HIPCHK(c, hipGetLastError());
    if ((rc = Pk.download())) return rc;   // status | best_pos | descriptors | normal, max | min: one copy back, one synchronisation
    memcpy(status, Pk.host(dst), nP);
    if (best_pos) memcpy(best_pos, Pk.host(dbest), nP * 4);
    if (desc_out) memcpy(desc_out, Pk.host(ddesc), nP * 32);
    const float *hB = (const float *)Pk.host(dB);
    for (size_t p = 0; p < nP && normal_out; p++) normal_out[3 * p] = hB[4 * p], normal_out[3 * p + 1] = hB[4 * p + 1], normal_out[3 * p + 2] = hB[4 * p + 2];
    for (size_t p = 0; p < nP && max_dist_out; p++) max_dist_out[p] = hB[4 * p + 3];
    if (min_dist_out) memcpy(min_dist_out, Pk.host(dmin), nP * 4);
    return ORBHIP_OK;
}

extern "C" int orbhip_map_get(orbhip_ctx *c, int n, const uint64_t *keys, float *pos, float *normal, float *min_dist, float *max_dist,
                              uint8_t *desc, uint8_t *flags)
{
    const char *who = "orbhip_map_get";
    if (!c || n < 0 || (n > 0 && !keys)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbLocalMap *M = lmap(c);
    if (!M) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no store (orbhip_map_init)");
    if (n == 0) return ORBHIP_OK;
    for (int i = 0; i < n; i++)
        if (!keys[i] || !M->slotOf.count(keys[i])) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a key is not in the store");
    HIPCHK(c, orb_enter(c));
    Packed Pk(c);
    int rc;
    const size_t nn = (size_t)n;
    if ((rc = Pk.begin(nn * (4 + 16 + 16 + 32 + 4) + 6 * 256))) return rc;
    int32_t *hs;
    const int32_t *ds = (const int32_t *)Pk.in_reserve(nn * 4, (void **)&hs);
    for (int i = 0; i < n; i++) hs[i] = M->slotOf.find(keys[i])->second;
    void *dA = Pk.out(nn * 16), *dB = Pk.out(nn * 16), *dD = Pk.out(nn * 32);
    uint32_t *dF = (uint32_t *)Pk.out(nn * 4);
    if ((rc = Pk.upload())) return rc;
    launch_map_gather(c->stream, ds, n, M->maxPoints, M->geoA.as<void>(), M->geoB.as<void>(), M->flags.as<uint32_t>(), M->desc.as<void>(),
                      dA, dB, dD, dF);
    HIPCHK(c, hipGetLastError());
    if ((rc = Pk.download())) return rc;
    const float *hA = (const float *)Pk.host(dA), *hB = (const float *)Pk.host(dB);
    const uint32_t *hF = (const uint32_t *)Pk.host(dF);
    for (size_t i = 0; i < nn; i++) {
        if (pos) pos[3 * i] = hA[4 * i], pos[3 * i + 1] = hA[4 * i + 1], pos[3 * i + 2] = hA[4 * i + 2];
        if (min_dist) min_dist[i] = hA[4 * i + 3];
        if (normal) normal[3 * i] = hB[4 * i], normal[3 * i + 1] = hB[4 * i + 1], normal[3 * i + 2] = hB[4 * i + 2];
        if (max_dist) max_dist[i] = hB[4 * i + 3];
        if (flags) flags[i] = (uint8_t)(hF[i] & (ORBHIP_MP_OBSERVED | ORBHIP_MP_BAD));
    }
    if (desc) memcpy(desc, Pk.host(dD), nn * 32);
    return ORBHIP_OK;
}
