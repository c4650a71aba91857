// api_baproblem.hip -- C ABI, part 17: the structure of Optimizer::LocalBundleAdjustment's problem from the resident key-frame
// table.  orbhip_map_ba_problem returns, for the local key frames of the call, the local map points
// (orbhip_map_collect's list, element for element), every point's observers over all live rows in ascending key-frame key as
// {kf, idx} edges in CSR form, and the fixed key frames in the order of their first edge (k_baproblem.hip).  It applies nothing
// and measures nothing: the caller reads mvKeysUn[idx] itself and hands the lists to its solver.  Every argument is checked
// before any device work; one upload of 8 B per local key frame and 8 B per table row, one result block, one synchronisation.
#include "localmap_store.h"

#define BA_MAX_KFS 65536

extern "C" int orbhip_map_ba_problem(orbhip_ctx *c, int nkf, const uint64_t *kf_keys, uint64_t *point_keys_out, int cap_points, int *npoints,
                                     int32_t *edge_off_out, orbhip_ba_edge *edges_out, int cap_edges, int *nedges,
                                     uint64_t *fixed_keys_out, int cap_fixed, int *nfixed)
{
    const char *who = "orbhip_map_ba_problem";
    if (!c || nkf < 0 || (nkf > 0 && !kf_keys) || cap_points < 0 || cap_edges < 0 || cap_fixed < 0 || (cap_points > 0 && !point_keys_out) ||
        (cap_edges > 0 && !edges_out) || (cap_fixed > 0 && !fixed_keys_out) || !edge_off_out || !npoints || !nedges || !nfixed)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (nkf > BA_MAX_KFS) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65536 key frames in one call");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    std::vector<int32_t> rowIdx;
    std::vector<uint32_t> off;
    int rc;
    if ((rc = kf_call_rows(c, K, who, nkf, kf_keys, rowIdx, off))) return rc;
    const uint32_t total = off[nkf];   // the local rows' entries: no call has more local points
    if (total == 0) {
        *npoints = *nedges = *nfixed = 0;
        edge_off_out[0] = 0;
        return ORBHIP_OK;
    }
    // every live row is an observer: the rank of its key (the order of a segment) and its place among the local key frames
    const int R = K->rowHigh;
    std::vector<std::pair<uint64_t, int32_t> > live;
    live.reserve(K->rowOf.size());
    uint64_t allEntries = 0;   // no call has more edges
    for (const auto &kv : K->rowOf) {
        live.push_back(std::make_pair(kv.first, kv.second));
        allEntries += K->entries[kv.second].size();
    }
    std::sort(live.begin(), live.end());
    const int boundP = (int)total;
    const uint32_t boundE = (uint32_t)allEntries;   // (<= KF_MAX_ENTRIES)
    const int capP = std::min(cap_points, boundP), capF = std::min(cap_fixed, R);
    const int capE = (int)std::min<uint64_t>((uint64_t)cap_edges, allEntries);
    HIPCHK(c, orb_enter(c));
    // scratch: cand | block counts | slots | {header, cnt, cursor} zero | off | firstPos ~0 | list | fixedRank | raw | sorted
    size_t at = 0;
    auto carve = [&at](size_t bytes) {
        const size_t a = at;
        at = align_up(at + bytes, 256);
        return a;
    };
    const size_t oCand = carve((size_t)total * 4), oBlk = carve((size_t)collect_blocks(total) * 4), oSlots = carve((size_t)total * 4);
    const size_t oZero = carve(256), oCnt = carve(((size_t)total + 1) * 4), oCur = carve((size_t)total * 4), oZeroEnd = at;
    const size_t oOff = carve(((size_t)total + 1) * 4), oFirst = carve((size_t)R * 4), oList = carve((size_t)R * 8);
    const size_t oRank = carve((size_t)R * 4), oRaw = carve((size_t)boundE * 8), oSorted = carve((size_t)boundE * 8);
    if (K->scratch.bytes() < at) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, K->scratch.grow(at, at + at / 2));
    }
    uint8_t *S = K->scratch.as<uint8_t>();
    int32_t *dhdr = (int32_t *)(S + oZero);
    Packed P(c);
    if ((rc = P.begin((size_t)nkf * 8 + 4 + (size_t)R * 8 + 256 + (size_t)capP * 8 + 4 + (size_t)capF * 4 + (size_t)capE * 8 + 10 * 256))) return rc;
    const int32_t *drowIdx = (const int32_t *)P.in(rowIdx.data(), (size_t)nkf * 4);
    const uint32_t *doff = (const uint32_t *)P.in(off.data(), (size_t)(nkf + 1) * 4);
    int32_t *hrank, *hlocal;
    const int32_t *drank = (const int32_t *)P.in_reserve((size_t)R * 4, (void **)&hrank);
    const int32_t *dlocal = (const int32_t *)P.in_reserve((size_t)R * 4, (void **)&hlocal);
    for (int r = 0; r < R; r++) hrank[r] = hlocal[r] = -1;
    for (size_t k = 0; k < live.size(); k++) hrank[live[k].second] = (int32_t)k;
    for (int k = nkf - 1; k >= 0; k--) hlocal[rowIdx[k]] = k;   // the first occurrence stays
    int32_t *rhdr = (int32_t *)P.out(256);
    int32_t *rslots = (int32_t *)P.out((size_t)capP * 4);
    int32_t *roff = (int32_t *)P.out(((size_t)capP + 1) * 4);
    int32_t *rfixed = (int32_t *)P.out((size_t)capF * 4);
    void *redges = P.out((size_t)capE * 8);
    if ((rc = P.upload())) return rc;
    HIPCHK(c, hipMemsetAsync(S + oZero, 0, oZeroEnd - oZero, c->stream));
    HIPCHK(c, hipMemsetAsync(S + oFirst, 0xFF, (size_t)R * 4, c->stream));
    launch_collect(c->stream, K->rows.as<void>(), R, K->stride, drowIdx, doff, nkf, total, M->flags.as<uint32_t>(), M->maxPoints,
                   K->marks.as<uint32_t>(), K->first.as<uint32_t>(), (int32_t *)(S + oCand), (int32_t *)(S + oBlk), boundP,
                   (int32_t *)(S + oSlots), nullptr, dhdr);
    launch_ba_problem(c->stream, K->rows.as<void>(), R, K->stride, K->maxRow, M->flags.as<uint32_t>(), M->maxPoints, K->marks.as<uint32_t>(),
                      drank, dlocal, nkf, dhdr, boundP, (const int32_t *)(S + oSlots), (uint32_t *)(S + oCnt), (uint32_t *)(S + oOff),
                      (uint32_t *)(S + oCur), S + oRaw, S + oSorted, boundE, (uint32_t *)(S + oFirst), S + oList, (int32_t *)(S + oRank), capP,
                      capE, capF, rhdr, rslots, roff, rfixed, redges);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download())) return rc;
    const int32_t *h = (const int32_t *)P.host(rhdr);
    const int np = h[0], ne = h[1], nf = h[2];
    if (np < 0 || np > boundP || ne < np || (uint64_t)ne > allEntries || nf < 0 || nf > (int)live.size() || h[3] != 0)
        return fail(c, ORBHIP_E_HIP, std::string(who) + ": internal: a count outside its bound");
    if (np > cap_points || ne > cap_edges || nf > cap_fixed) {
        *npoints = np, *nedges = ne, *nfixed = nf;
        return fail(c, ORBHIP_E_CAPACITY, std::string(who) + ": more points, edges or fixed key frames than room (the counts have the numbers)");
    }
    const int32_t *hs = (const int32_t *)P.host(rslots), *ho = (const int32_t *)P.host(roff), *hf = (const int32_t *)P.host(rfixed);
    const orbhip_ba_edge *he = (const orbhip_ba_edge *)P.host(redges);
    bool ok = ho[0] == 0 && ho[np] == ne;
    for (int j = 0; j < np && ok; j++) ok = hs[j] >= 0 && hs[j] < M->maxPoints && M->slotKey[hs[j]] != 0 && ho[j + 1] > ho[j];
    for (int r = 0; r < nf && ok; r++) ok = hf[r] >= 0 && hf[r] < R && K->rowKey[hf[r]] != 0;
    for (int p = 0; p < ne && ok; p++) ok = he[p].kf >= 0 && he[p].kf < nkf + nf && he[p].idx >= 0 && he[p].idx < K->maxRow;
    if (!ok) return fail(c, ORBHIP_E_HIP, std::string(who) + ": internal: a result outside the table");
    *npoints = np, *nedges = ne, *nfixed = nf;
    for (int j = 0; j < np; j++) point_keys_out[j] = M->slotKey[hs[j]];
    memcpy(edge_off_out, ho, ((size_t)np + 1) * 4);
    if (ne) memcpy(edges_out, he, (size_t)ne * sizeof(orbhip_ba_edge));
    for (int r = 0; r < nf; r++) fixed_keys_out[r] = K->rowKey[hf[r]];
    return ORBHIP_OK;
}
