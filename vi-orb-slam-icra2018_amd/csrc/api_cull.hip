// api_cull.hip -- C ABI, part 16: the counts of LocalMapping::KeyFrameCulling from the resident key-frame table (DESIGN.md section
// 22).  orbhip_map_kf_levels keeps one byte per row entry (octave, "counts twice in nObs", "far") in a device array parallel to the
// rows; orbhip_map_cull counts, for a batch of candidate key frames on the map as it is, the points that count and the redundant
// ones (k_cull.hip) and forms the reference's nRedundantObservations>0.9*nMPs on the host.  It applies nothing: a cull changes the
// counts of every later candidate, so the caller culls one key frame at a time and counts again (LocalMapCull.cc).  Every argument
// is checked before any device work; one upload of 8 B per candidate, one result block, one synchronisation.
#include "localmap_store.h"

#define CULL_MAX_CANDIDATES 65536
#define CULL_COLS 17   // k_cull.hip: the tally's columns

static bool kf_levels_current(const OrbKfTable *K, int row) { return K->levelsN[row] >= (int32_t)K->entries[row].size(); }

extern "C" int orbhip_map_kf_levels(orbhip_ctx *c, int m, const uint64_t *kf_keys, const int32_t *off, const uint8_t *bytes)
{
    const char *who = "orbhip_map_kf_levels";
    if (!c || m < 0 || (m > 0 && (!kf_keys || !off))) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    if (m == 0) return ORBHIP_OK;
    if (off[0] != 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": off does not start at 0");
    std::vector<int32_t> desc((size_t)m * 3);
    {
        std::vector<uint64_t> seen(kf_keys, kf_keys + m);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a key frame twice in the call");
    }
    for (int q = 0; q < m; q++) {
        auto it = K->rowOf.find(kf_keys[q]);
        if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame");
        if (off[q + 1] < off[q]) return fail(c, ORBHIP_E_ARG, std::string(who) + ": off does not ascend");
        if (off[q + 1] - off[q] > K->maxRow) return fail(c, ORBHIP_E_ARG, std::string(who) + ": a segment longer than max_row (orbhip_map_kf_init)");
        desc[3 * q] = it->second, desc[3 * q + 1] = off[q], desc[3 * q + 2] = off[q + 1] - off[q];
    }
    const int total = off[m];
    if (total > 0 && !bytes) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    for (int i = 0; i < total; i++)
        if (bytes[i] & 0x30) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bit 4 or 5 of a level byte is set");
    HIPCHK(c, orb_enter(c));
    const size_t all = (size_t)K->maxKfs * K->maxRow;
    if (!K->levels) {   // the first put of levels: later ones allocate nothing
        HIPCHK(c, K->levels.grow(all));
        HIPCHK(c, hipMemsetAsync(K->levels.as<void>(), 0, all, c->stream));
    }
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)total + (size_t)m * 12 + 3 * 256))) return rc;
    const uint8_t *db = (const uint8_t *)P.in(bytes, (size_t)total);
    const int32_t *dd = (const int32_t *)P.in(desc.data(), (size_t)m * 12);
    if ((rc = P.upload())) return rc;
    launch_cull_levels(c->stream, db, dd, m, K->maxKfs, K->maxRow, K->levels.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < m; q++) K->levelsN[desc[3 * q]] = desc[3 * q + 2];
    return ORBHIP_OK;
}

extern "C" int orbhip_map_kf_levels_missing(orbhip_ctx *c, uint64_t *kf_keys_out, int cap, int *nout)
{
    const char *who = "orbhip_map_kf_levels_missing";
    if (!c || cap < 0 || (cap > 0 && !kf_keys_out) || !nout) return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    *nout = 0;
    OrbKfTable *K = kf_table(c);
    if (!K) return ORBHIP_OK;
    std::vector<uint64_t> v;
    for (const auto &kv : K->rowOf)
        if (!kf_levels_current(K, kv.second)) v.push_back(kv.first);
    std::sort(v.begin(), v.end());
    *nout = (int)v.size();
    for (int k = 0; k < (int)v.size() && k < cap; k++) kf_keys_out[k] = v[k];
    if ((int)v.size() > cap) return fail(c, ORBHIP_E_CAPACITY, std::string(who) + ": more key frames than cap (*nout has the number)");
    return ORBHIP_OK;
}

extern "C" int orbhip_map_cull(orbhip_ctx *c, int Kc, const uint64_t *kf_keys, int monocular, int th_obs, orbhip_cull_count *counts,
                               uint8_t *redundant, uint8_t *entry_state)
{
    const char *who = "orbhip_map_cull";
    if (!c || Kc < 0 || (Kc > 0 && (!kf_keys || !counts || !redundant)) || th_obs < 1)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (Kc > CULL_MAX_CANDIDATES) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65536 key frames in one call");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    if (Kc == 0) return ORBHIP_OK;
    std::vector<int32_t> cand((size_t)Kc * 2);   // {row, length}
    uint64_t bound = 0;                          // the candidates' row entries: no call claims more ids
    for (int k = 0; k < Kc; k++) {
        auto it = K->rowOf.find(kf_keys[k]);
        if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame");
        cand[2 * k] = it->second, cand[2 * k + 1] = (int32_t)K->entries[it->second].size();
        bound += K->entries[it->second].size();
    }
    for (const auto &kv : K->rowOf)   // every live row is an observer: its octaves are read
        if (!kf_levels_current(K, kv.second))
            return fail(c, ORBHIP_E_ARG, std::string(who) + ": a key frame of the table has no levels, or fewer than its row (orbhip_map_kf_levels)");
    if (bound > KF_MAX_CALL) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": more than 2^24 row entries in one call");
    HIPCHK(c, orb_enter(c));
    // scratch: the id counter | tally [bound][17]
    const size_t tallyBytes = (size_t)bound * CULL_COLS * 4, need = 256 + tallyBytes + 256;
    if (K->scratch.bytes() < need) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, K->scratch.grow(need, need + need / 2));
    }
    uint32_t *dnids = K->scratch.as<uint32_t>(), *dtally = (uint32_t *)(K->scratch.as<uint8_t>() + 256);
    const size_t stateBytes = entry_state ? (size_t)Kc * K->maxRow : 0;
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)Kc * 16 + stateBytes + 4 * 256))) return rc;
    const void *dcand = P.in(cand.data(), (size_t)Kc * 8);
    void *dcounts = P.out((size_t)Kc * 8);
    uint8_t *dstate = entry_state ? (uint8_t *)P.out(stateBytes) : nullptr;
    if ((rc = P.upload())) return rc;
    HIPCHK(c, hipMemsetAsync(K->scratch.as<void>(), 0, 256 + tallyBytes, c->stream));
    launch_cull(c->stream, K->rows.as<void>(), K->rowHigh, K->stride, K->maxRow, K->levels.as<uint8_t>(), M->flags.as<uint32_t>(),
                M->maxPoints, K->marks.as<uint32_t>(), dcand, Kc, (uint32_t)bound, dnids, dtally, monocular != 0, th_obs, dcounts, dstate);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    const int32_t *h = (const int32_t *)P.host(dcounts);
    for (int k = 0; k < Kc; k++)
        if (h[2 * k] < 0 || h[2 * k] > cand[2 * k + 1] || h[2 * k + 1] < 0 || h[2 * k + 1] > h[2 * k])
            return fail(c, ORBHIP_E_HIP, std::string(who) + ": internal: a count outside its row");
    for (int k = 0; k < Kc; k++) {
        const int nMPs = h[2 * k], nRedundantObservations = h[2 * k + 1];
        counts[k].n_mps = nMPs, counts[k].n_redundant = nRedundantObservations;
        redundant[k] = (double)nRedundantObservations > 0.9 * (double)nMPs;   // ref: src/LocalMapping.cc:1581
    }
    if (entry_state) memcpy(entry_state, P.host(dstate), stateBytes);
    return ORBHIP_OK;
}
