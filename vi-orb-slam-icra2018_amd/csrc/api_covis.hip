// api_covis.hip -- C ABI, part 14: the covisibility graph from the resident key-frame table.
// orbhip_map_covis: the counting loop of KeyFrame::UpdateConnections (ref: src/KeyFrame.cc:731-765) for a batch of key frames in
// sweeps of the table (k_covis.hip: 32 queries per sweep), then the rules that turn the counts into mConnectedKeyFrameWeights and
// the ordered lists (:767-812) on the host, where the row -> key mapping lives.  Every argument is checked before any device
// work; one packed upload, the passes enqueued back to back, one result block, one synchronisation.
#include "localmap_store.h"

#define COVIS_MAX_QUERIES 65536
#define COVIS_MAX_PAIRS ((int64_t)1 << 30)   // queries * live rows of one call: the device counts the links in an int32

extern "C" int orbhip_map_covis(orbhip_ctx *c, int nq, const uint64_t *kf_keys, int th, int32_t *off_out, uint64_t *nbr_keys_out,
                                int32_t *weights_out, int32_t *order_out, int32_t *nordered_out, int cap, int *ntotal)
{
    const char *who = "orbhip_map_covis";
    if (!c || nq < 0 || (nq > 0 && (!kf_keys || !nordered_out)) || th < 1 || !off_out || cap < 0 ||
        (cap > 0 && (!nbr_keys_out || !weights_out || !order_out)) || !ntotal)
        return fail(c, ORBHIP_E_ARG, std::string(who) + ": bad argument");
    if (nq > COVIS_MAX_QUERIES) return fail(c, ORBHIP_E_ARG, std::string(who) + ": more than 65536 key frames in one call");
    OrbLocalMap *M = lmap(c);
    OrbKfTable *K = kf_table(c);
    if (!K) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no table (orbhip_map_kf_init)");
    std::vector<int32_t> qrow(nq);
    for (int q = 0; q < nq; q++) {
        auto it = K->rowOf.find(kf_keys[q]);
        if (it == K->rowOf.end()) return fail(c, ORBHIP_E_ARG, std::string(who) + ": unknown key frame");
        qrow[q] = it->second;
    }
    if (nq == 0) {
        off_out[0] = 0;
        *ntotal = 0;
        return ORBHIP_OK;
    }
    const int64_t pairs = (int64_t)nq * (int64_t)K->rowOf.size();
    if (pairs > COVIS_MAX_PAIRS) return fail(c, ORBHIP_E_SIZE, std::string(who) + ": queries times live key frames above 2^30");
    HIPCHK(c, orb_enter(c));
    const int R = K->rowHigh, capDev = (int)std::min<int64_t>(cap, pairs);
    Packed P(c);
    int rc;
    if ((rc = P.begin((size_t)nq * 4 + 16 + (size_t)capDev * 8 + 4 * 256))) return rc;
    const int32_t *dq = (const int32_t *)P.in(qrow.data(), (size_t)nq * 4);
    const int32_t zero[4] = {0, 0, 0, 0};
    int32_t *dn = (int32_t *)P.in(zero, 16);   // the count (comes back with the triples behind it)
    int32_t *dtrip = (int32_t *)P.out((size_t)capDev * 8);
    if ((rc = P.upload())) return rc;
    launch_covis(c->stream, K->rows.as<void>(), R, K->stride, K->maxRow, M->flags.as<uint32_t>(), M->maxPoints, K->marks.as<uint32_t>(),
                 dq, nq, capDev, dn, dtrip);
    HIPCHK(c, hipGetLastError());
    if ((rc = P.download(dn))) return rc;
    const int total = *(const int32_t *)P.host(dn);
    if (total < 0 || (int64_t)total > pairs) return fail(c, ORBHIP_E_HIP, std::string(who) + ": internal: link count out of range");
    if (total > cap) {
        *ntotal = total;
        return fail(c, ORBHIP_E_CAPACITY, std::string(who) + ": more links than cap (*ntotal has the number)");
    }
    // (query, key, weight) in ascending (query, key): KFcounter of every query in the canonical order (docs/parity.md)
    struct Link {
        int32_t q;
        uint64_t key;
        int32_t w;
    };
    const int32_t *h = (const int32_t *)P.host(dtrip);
    std::vector<Link> v(total);
    for (int k = 0; k < total; k++) {
        const uint32_t a = (uint32_t)h[2 * k];
        const int row = (int)(a & 0xFFFFu), q = (int)(a >> 16);
        if (q >= nq || row >= K->maxKfs || !K->rowKey[row] || h[2 * k + 1] <= 0)
            return fail(c, ORBHIP_E_HIP, std::string(who) + ": internal: a link outside the call");
        v[k].q = q, v[k].key = K->rowKey[row], v[k].w = h[2 * k + 1];
    }
    std::sort(v.begin(), v.end(), [](const Link &a, const Link &b) { return a.q != b.q ? a.q < b.q : a.key < b.key; });
    *ntotal = total;
    std::vector<int32_t> sel;
    int k = 0;
    for (int q = 0; q < nq; q++) {
        const int beg = k;
        off_out[q] = beg;
        while (k < total && v[k].q == q) nbr_keys_out[k] = v[k].key, weights_out[k] = v[k].w, k++;
        // the links of weight >= th, or the first maximum in ascending key order (if(mit->second>nmax)); then descending weight,
        // ties by descending key: sort(vector<pair<int, KeyFrame*>>) read from the back
        sel.clear();
        int best = -1;
        for (int i = beg; i < k; i++) {
            if (v[i].w >= th) sel.push_back(i - beg);
            if (best < 0 || v[i].w > v[best].w) best = i;
        }
        if (sel.empty() && best >= 0) sel.push_back(best - beg);
        std::sort(sel.begin(), sel.end(), [&](int32_t a, int32_t b) {
            const Link &x = v[beg + a], &y = v[beg + b];
            return x.w != y.w ? x.w > y.w : x.key > y.key;
        });
        nordered_out[q] = (int32_t)sel.size();
        for (size_t r = 0; r < sel.size(); r++) order_out[beg + r] = sel[r];
    }
    off_out[nq] = total;
    return ORBHIP_OK;
}
