// mock_sim3search.cc -- the host model of the entry points ORB_SLAM2::LocalMapSearch calls (tests/native_fuse/mock_fuse.cc: store,
// key-frame table with incarnations, sets) with orbhip_search_by_sim3 modelled on top of it, for the programs that run
// LocalMapSearch::SearchBySim3 without a device (test_sim3search_mock, test_sim3search_mock_asan): the projection of ref_sim3.h over
// the store's copies of the points, the oracle's ungated window search and the agreement.  mock_sim3_calls() counts the calls, and
// mock_sim3_fail_next() makes the next one fail, for the program's -1 paths.
#include "../native_fuse/mock_fuse.cc"
#include "ref_sim3.h"

namespace
{
int g_calls = 0;
bool g_failNext = false;
}  // namespace

extern "C" {
int mock_sim3_calls() { return g_calls; }
void mock_sim3_fail_next() { g_failNext = true; }

int orbhip_search_by_sim3(orbhip_ctx *, const orbhip_fuse_target *sides, const uint64_t *row_keys, const float *sR21, const float *t21,
                          const float *sR12, const float *t12, float th, int th_high, const uint8_t *taken1, const uint8_t *taken2,
                          int32_t *match12, int *nfound, int32_t *n_active, orbhip_proj_query *queries1_out, int32_t *best1, int32_t *dist1,
                          orbhip_proj_query *queries2_out, int32_t *best2, int32_t *dist2)
{
    g_calls++;
    if (g_failNext) return g_failNext = false, ORBHIP_E_HIP;
    if (!std::isfinite(th)) return ORBHIP_E_ARG;
    for (int s = 0; s < 2; s++) {
        if (!g.rows.count(row_keys[s]) || !g.sets.count(sides[s].set_key) || !g.sets[sides[s].set_key].grid) return ORBHIP_E_ARG;
        if (sides[s].cam.nlevels < 1 || sides[s].cam.nlevels > 16) return ORBHIP_E_ARG;
        if (g.rows[row_keys[s]].size() != g.sets[sides[s].set_key].kps.size()) return ORBHIP_E_ARG;
    }
    const reffuse::Camera cam[2] = {camera_of(&sides[0].cam), camera_of(&sides[1].cam)};
    const uint8_t *taken[2] = {taken1, taken2};
    std::vector<int32_t> best[2], dist[2];
    std::vector<orbo_proj_query> q[2];
    for (int d = 0; d < 2; d++) {
        const Row &row = g.rows[row_keys[d]];
        const int n = (int)row.size();
        const Set &S = g.sets[sides[1 - d].set_key];
        q[d].resize(n), best[d].assign(n, -1), dist[d].assign(n, 256);
        std::vector<uint8_t> qdesc((size_t)n * 32, 0);
        n_active[d] = 0;
        for (int i = 0; i < n; i++) {
            memset(&q[d][i], 0, sizeof q[d][i]);
            const Point *p = (taken[d] && taken[d][i]) ? NULL : resolve(row[i]);
            if (!p) continue;
            if (refsim3::sim3_query(cam[d], d == 0 ? sR21 : sR12, d == 0 ? t21 : t12, cam[0], cam[1 - d], th, p->pos, p->mn, p->mx, &q[d][i])) {
                memcpy(&qdesc[(size_t)i * 32], p->desc, 32);
                n_active[d]++;
            }
        }
        if (n)
            orbo_window_best(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), (int)S.kps.size(), NULL, NULL, S.gp[0], S.gp[1],
                             S.gp[2], S.gp[3], q[d].data(), qdesc.data(), n, best[d].data(), dist[d].data());
    }
    std::vector<int32_t> m;
    *nfound = refsim3::agree(best[0], dist[0], best[1], dist[1], th_high, m);
    memcpy(match12, m.data(), m.size() * 4);
    orbhip_proj_query *qo[2] = {queries1_out, queries2_out};
    int32_t *bo[2] = {best1, best2}, *eo[2] = {dist1, dist2};
    for (int d = 0; d < 2; d++) {
        if (qo[d]) memcpy(qo[d], q[d].data(), q[d].size() * sizeof(orbo_proj_query));
        if (bo[d]) memcpy(bo[d], best[d].data(), best[d].size() * 4);
        if (eo[d]) memcpy(eo[d], dist[d].data(), dist[d].size() * 4);
    }
    return ORBHIP_OK;
}
}
