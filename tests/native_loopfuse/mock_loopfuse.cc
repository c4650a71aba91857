// mock_loopfuse.cc -- the host model of the entry points ORB_SLAM2::LocalMapSearch calls (tests/native_fuse/mock_fuse.cc: store,
// key-frame table with incarnations, sets) with the three entry points of LoopClosing's searches modelled on top of it, for the
// programs that run SearchLoopPoints and SearchAndFuse without a device (test_loopfuse_mock, test_loopfuse_mock_asan):
// orbhip_fuse_sim3 and orbhip_search_loop_points are the projection of ref_loop.h over the store's copies of the points with the
// oracle's ungated window search, respectively its sequential claim, behind it; orbhip_map_kf_set_batch edits the table's rows
// all or nothing.  mock_state_digest() is a digest of everything the store and the table hold, for the program's comparison with
// a fresh Put / PutKeyFrame of every object.
#include "../native_fuse/mock_fuse.cc"

namespace
{
// the queries of the points `pts` (NULL: inactive) in one target; proj_xr = 0
int project_sim3(const orbhip_fuse_target &t, const std::vector<const Point *> &pts, std::vector<orbo_proj_query> &q, std::vector<uint8_t> &qdesc)
{
    const reffuse::Camera C = camera_of(&t.cam);
    const int n = (int)pts.size();
    q.resize(n), qdesc.assign((size_t)n * 32, 0);
    int active = 0;
    for (int i = 0; i < n; i++) {
        memset(&q[i], 0, sizeof q[i]);
        if (!pts[i]) continue;
        if (reffuse::fuse_query(C, pts[i]->pos, pts[i]->nrm, pts[i]->mn, pts[i]->mx, &q[i])) {
            memcpy(&qdesc[(size_t)i * 32], pts[i]->desc, 32);
            active++;
        }
        q[i].proj_xr = 0;
    }
    return active;
}
}  // namespace

extern "C" {
int orbhip_map_kf_set_batch(orbhip_ctx *, int m, const uint64_t *kf_keys, const int32_t *idx, const uint64_t *point_keys)
{
    std::map<uint64_t, Row> after;
    std::set<std::pair<uint64_t, int32_t> > named;
    for (int j = 0; j < m; j++) {
        if (!g.rows.count(kf_keys[j])) return ORBHIP_E_ARG;
        if (!after.count(kf_keys[j])) after[kf_keys[j]] = g.rows[kf_keys[j]];
        Row &row = after[kf_keys[j]];
        if (idx[j] < 0 || idx[j] >= (int)row.size() || (point_keys[j] && !g.points.count(point_keys[j]))) return ORBHIP_E_ARG;
        if (!named.insert(std::make_pair(kf_keys[j], idx[j])).second) return ORBHIP_E_ARG;
        row[idx[j]] = std::make_pair(point_keys[j], point_keys[j] ? g.incarnation[point_keys[j]] : 0u);
    }
    for (auto &kv : after) {
        std::set<uint64_t> seen;
        for (size_t i = 0; i < kv.second.size(); i++)
            if (kv.second[i].first && !seen.insert(kv.second[i].first).second) return ORBHIP_E_ARG;
    }
    for (auto &kv : after) g.rows[kv.first] = kv.second;
    return ORBHIP_OK;
}

int orbhip_fuse_sim3(orbhip_ctx *, const orbhip_fuse_target *targets, const uint64_t *target_row_keys, int K, const uint64_t *point_keys, int n,
                     orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist, int32_t *n_active)
{
    if (K < 0 || n < 0) return ORBHIP_E_ARG;
    if (K == 0) return ORBHIP_OK;
    std::set<uint64_t> distinct, seen;
    for (int k = 0; k < K; k++) {
        if (!target_ok(targets[k]) || (target_row_keys && target_row_keys[k] && !g.rows.count(target_row_keys[k]))) return ORBHIP_E_ARG;
        distinct.insert(targets[k].set_key);
    }
    if ((int)distinct.size() > g.setLimit) return ORBHIP_E_ARG;
    for (int i = 0; i < n; i++)
        if (point_keys[i] && !seen.insert(point_keys[i]).second) return ORBHIP_E_ARG;
    std::vector<orbo_proj_query> q;
    std::vector<uint8_t> qdesc;
    for (int k = 0; k < K; k++) {
        std::set<uint64_t> held;                  // spAlreadyFound: what the target's row resolves to (live, the entry's incarnation, not bad)
        if (target_row_keys && target_row_keys[k]) {
            const Row &row = g.rows[target_row_keys[k]];
            for (size_t i = 0; i < row.size(); i++)
                if (resolve(row[i])) held.insert(row[i].first);
        }
        std::vector<const Point *> pts(n, (const Point *)NULL);
        for (int i = 0; i < n; i++) {
            auto it = point_keys[i] ? g.points.find(point_keys[i]) : g.points.end();
            if (it != g.points.end() && !(it->second.flags & ORBHIP_MP_BAD) && !held.count(point_keys[i])) pts[i] = &it->second;
        }
        n_active[k] = project_sim3(targets[k], pts, q, qdesc);
        const Set &S = g.sets[targets[k].set_key];
        if (n)
            orbo_window_best(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), (int)S.kps.size(), NULL, NULL, S.gp[0], S.gp[1],
                             S.gp[2], S.gp[3], q.data(), qdesc.data(), n, best_idx + (size_t)k * n, best_dist + (size_t)k * n);
        if (queries_out && n) memcpy(queries_out + (size_t)k * n, q.data(), (size_t)n * sizeof(orbo_proj_query));
    }
    return ORBHIP_OK;
}

int orbhip_search_loop_points(orbhip_ctx *c, const orbhip_fuse_target *target, int nkf, const uint64_t *kf_keys, const uint64_t *matched_keys,
                              int th_high, uint64_t *keys_out, int cap, int *npoints, orbhip_proj_query *queries_out, int *n_active,
                              int32_t *match, int *nmatches)
{
    if (!target_ok(*target)) return ORBHIP_E_ARG;
    for (int k = 0; k < nkf; k++)
        if (!g.rows.count(kf_keys[k])) return ORBHIP_E_ARG;
    const Set &S = g.sets[target->set_key];
    const int nf = (int)S.kps.size();
    std::vector<uint64_t> keys(cap > 0 ? cap : 1);
    int n = 0;
    const int rc = orbhip_map_collect(c, nkf, kf_keys, keys.data(), cap, &n);
    *npoints = n, *n_active = 0, *nmatches = 0;
    for (int i = 0; i < nf; i++) match[i] = -1;
    for (int i = 0; i < n && i < cap; i++) keys_out[i] = keys[i];
    if (rc != ORBHIP_OK) return rc;
    std::set<uint64_t> found;
    std::vector<uint8_t> occupied(nf > 0 ? nf : 1, 0);
    for (int i = 0; i < nf && matched_keys; i++)
        if (matched_keys[i]) found.insert(matched_keys[i]), occupied[i] = 1;
    std::vector<const Point *> pts(n);
    for (int i = 0; i < n; i++) pts[i] = found.count(keys[i]) ? NULL : &g.points[keys[i]];
    std::vector<orbo_proj_query> q;
    std::vector<uint8_t> qdesc;
    *n_active = project_sim3(*target, pts, q, qdesc);
    if (n && nf)
        *nmatches = orbo_search_by_projection(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), nf, NULL, occupied.data(),
                                              S.gp[0], S.gp[1], S.gp[2], S.gp[3], q.data(), qdesc.data(), n, 0, 0.f, 0, th_high, match);
    if (queries_out && n) memcpy(queries_out, q.data(), (size_t)n * sizeof(orbo_proj_query));
    return ORBHIP_OK;
}

unsigned long long mock_state_digest()
{
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&h](unsigned long long v) { h = (h ^ v) * 1099511628211ull; };
    for (auto &kv : g.points) {
        mix(kv.first), mix(kv.second.flags);
        unsigned long long w[8] = {0};
        memcpy(w, kv.second.pos, 12), memcpy((char *)w + 12, kv.second.nrm, 12), memcpy((char *)w + 24, &kv.second.mn, 4),
            memcpy((char *)w + 28, &kv.second.mx, 4), memcpy((char *)w + 32, kv.second.desc, 32);
        for (int k = 0; k < 8; k++) mix(w[k]);
    }
    for (auto &kv : g.rows) {
        mix(kv.first), mix(kv.second.size());
        for (size_t i = 0; i < kv.second.size(); i++) mix(resolve(kv.second[i]) ? kv.second[i].first : 0);
    }
    return h;
}
}
