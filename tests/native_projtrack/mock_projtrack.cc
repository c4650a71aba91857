// mock_projtrack.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch calls, for the programs that run its two
// projection searches without a device (test_projtrack_mock, test_projtrack_mock_asan): the store keeps what orbhip_map_put
// was given, the key-frame table keeps keys with the point's incarnation (an erased point's entries never resolve again, as the
// device's generation count has it), the sets keep keypoints and descriptors, and the two searches are the loops of
// ref_projtrack.h over those copies with the oracle's window search behind them.  The entry points the class links but these
// programs never reach (vote, collect, the local-points searches) fail loudly.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "orbhip.h"
#include "ref_projtrack.h"

namespace
{
struct Point {
    float pos[3], mn, mx;
    uint8_t desc[32], flags;
};
struct Set {
    std::vector<orbhip_keypoint> kps;
    std::vector<uint8_t> desc;
    float gp[4];
    bool grid;
};
struct Mock {
    int maxPoints = 0, maxKfs = 0, maxRow = 0;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, unsigned> incarnation;                              // key -> how often it was erased
    std::map<uint64_t, Set> sets;
    std::map<uint64_t, std::vector<std::pair<uint64_t, unsigned> > > rows; // kf -> (point key, incarnation at the time)
} g;

refpt::Camera camera_of(const orbhip_local_camera *c)
{
    refpt::Camera C;
    memset(&C, 0, sizeof C);
    memcpy(C.R, c->Rcw, sizeof C.R), memcpy(C.t, c->tcw, sizeof C.t), memcpy(C.Ow, c->Ow, sizeof C.Ow);
    C.fx = c->fx, C.fy = c->fy, C.cx = c->cx, C.cy = c->cy, C.mbf = c->mbf;
    C.minX = c->min_x, C.maxX = c->max_x, C.minY = c->min_y, C.maxY = c->max_y;
    memcpy(C.sf, c->scale_factors, sizeof C.sf);
    C.logS = c->log_scale_factor, C.th = c->th, C.nlevels = c->nlevels;
    return C;
}

int search(const Set &S, const float *u_right, const uint8_t *occupied, const std::vector<orbo_proj_query> &q,
           const std::vector<uint8_t> &qdesc, int check_ori, int th_high, int32_t *match)
{
    return orbo_search_by_projection(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), (int)S.kps.size(), u_right,
                                     occupied, S.gp[0], S.gp[1], S.gp[2], S.gp[3], q.data(), qdesc.data(), (int)q.size(), 0, 0.f,
                                     check_ori, th_high, match);
}
int unreachable(const char *who)
{
    fprintf(stderr, "mock_projtrack: %s is not modelled\n", who);
    return ORBHIP_E_ARG;
}
}  // namespace

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return (orbhip_ctx *)&g; }
void orbhip_destroy(orbhip_ctx *) {}
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g = Mock(); g.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *)
{
    for (auto &kv : g.points) g.incarnation[kv.first]++;
    g.points.clear();
    return ORBHIP_OK;
}
int orbhip_set_limit(orbhip_ctx *, int n) { return n; }
int orbhip_set_drop(orbhip_ctx *, uint64_t key)
{
    if (key) g.sets.erase(key); else g.sets.clear();
    return ORBHIP_OK;
}
int orbhip_set_has(orbhip_ctx *, uint64_t key, int n) { return g.sets.count(key) && (int)g.sets[key].kps.size() == n; }
int orbhip_set_info(orbhip_ctx *, uint64_t key, int *n, int *ng, uint64_t *fp)
{
    if (!g.sets.count(key)) return 0;
    if (n) *n = (int)g.sets[key].kps.size();
    if (ng) *ng = 0;
    if (fp) *fp = 0;   // (never equal to a fingerprint of data: the set is put again, which is always right)
    return 1;
}
uint64_t orbhip_set_fingerprint_rows(const orbhip_keypoint *, const uint8_t *, const uint8_t *, int n) { return 0x9E3779B97F4A7C15ull ^ (uint64_t)n; }
uint64_t orbhip_frame_fingerprint(const orbhip_ctx *) { return 0; }
int orbhip_set_put_from_frame(orbhip_ctx *, uint64_t, orbhip_ctx *, const int32_t *, const int32_t *, const int32_t *, int) { return unreachable("orbhip_set_put_from_frame"); }
int orbhip_set_put(orbhip_ctx *, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *, const int32_t *,
                   const int32_t *, int, float min_x, float min_y, float inv_w, float inv_h)
{
    if (!key || n <= 0) return ORBHIP_E_ARG;
    Set &S = g.sets[key];
    S.kps.assign(kps, kps + n);
    S.desc.assign(desc, desc + (size_t)n * 32);
    S.gp[0] = min_x, S.gp[1] = min_y, S.gp[2] = inv_w, S.gp[3] = inv_h;
    S.grid = inv_w > 0 && inv_h > 0;
    return ORBHIP_OK;
}
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *pos, const float *, const float *mn, const float *mx,
                   const uint8_t *desc, const uint8_t *flags)
{
    std::set<uint64_t> seen;
    size_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!keys[i] || !seen.insert(keys[i]).second) return ORBHIP_E_ARG;
        fresh += g.points.count(keys[i]) ? 0 : 1;
    }
    if (g.points.size() + fresh > (size_t)g.maxPoints) return ORBHIP_E_CAPACITY;
    for (int i = 0; i < n; i++) {
        Point &P = g.points[keys[i]];
        memcpy(P.pos, pos + 3 * i, 12);
        P.mn = mn[i], P.mx = mx[i], P.flags = flags[i];
        memcpy(P.desc, desc + 32 * (size_t)i, 32);
    }
    return ORBHIP_OK;
}
int orbhip_map_update_flags(orbhip_ctx *, int n, const uint64_t *keys, const uint8_t *flags)
{
    for (int i = 0; i < n; i++)
        if (!g.points.count(keys[i])) return ORBHIP_E_ARG;
    for (int i = 0; i < n; i++) g.points[keys[i]].flags = flags[i];
    return ORBHIP_OK;
}
int orbhip_map_erase(orbhip_ctx *, int n, const uint64_t *keys)
{
    for (int i = 0; i < n; i++)
        if (g.points.erase(keys[i])) g.incarnation[keys[i]]++;
    return ORBHIP_OK;
}
int orbhip_map_kf_init(orbhip_ctx *, int max_kfs, int max_row) { g.maxKfs = max_kfs, g.maxRow = max_row; g.rows.clear(); return ORBHIP_OK; }
int orbhip_map_kf_clear(orbhip_ctx *) { g.rows.clear(); return ORBHIP_OK; }
int orbhip_map_kf_put(orbhip_ctx *, uint64_t kf_key, int n, const uint64_t *point_keys)
{
    if (!kf_key || n > g.maxRow) return ORBHIP_E_ARG;
    std::vector<std::pair<uint64_t, unsigned> > row(n);
    for (int i = 0; i < n; i++) {
        if (point_keys[i] && !g.points.count(point_keys[i])) return ORBHIP_E_ARG;
        row[i] = std::make_pair(point_keys[i], point_keys[i] ? g.incarnation[point_keys[i]] : 0u);
    }
    g.rows[kf_key] = row;
    return ORBHIP_OK;
}
int orbhip_map_kf_set(orbhip_ctx *, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys)
{
    if (!g.rows.count(kf_key)) return ORBHIP_E_ARG;
    std::vector<std::pair<uint64_t, unsigned> > &row = g.rows[kf_key];
    for (int j = 0; j < m; j++) {
        if (idx[j] < 0 || idx[j] >= (int)row.size() || (point_keys[j] && !g.points.count(point_keys[j]))) return ORBHIP_E_ARG;
        row[idx[j]] = std::make_pair(point_keys[j], point_keys[j] ? g.incarnation[point_keys[j]] : 0u);
    }
    return ORBHIP_OK;
}
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t kf_key) { g.rows.erase(kf_key); return ORBHIP_OK; }

int orbhip_search_last_frame(orbhip_ctx *, uint64_t cur_key, uint64_t last_key, const uint64_t *last_point_keys, int n_last,
                             const orbhip_local_camera *cam, int motion, const float *u_right, const uint8_t *occupied, int check_ori,
                             int th_high, orbhip_proj_query *queries_out, int *n_active, int32_t *match, int *nmatches)
{
    if (!g.sets.count(cur_key) || !g.sets[cur_key].grid || (last_key && !g.sets.count(last_key)) || motion < 0 || motion > 2 ||
        cam->nlevels < 1 || cam->nlevels > 16)
        return ORBHIP_E_ARG;
    const Set &S = g.sets[cur_key];
    if (n_last != (last_key ? (int)g.sets[last_key].kps.size() : 0)) return ORBHIP_E_ARG;
    const refpt::Camera C = camera_of(cam);
    std::vector<orbo_proj_query> q(n_last);
    std::vector<uint8_t> qdesc((size_t)n_last * 32, 0);
    int active = 0;
    for (int i = 0; i < n_last; i++) {
        memset(&q[i], 0, sizeof q[i]);
        auto it = g.points.find(last_point_keys[i]);
        if (!last_point_keys[i] || it == g.points.end()) continue;
        const orbhip_keypoint &kp = g.sets[last_key].kps[i];
        if (refpt::last_query(C, it->second.pos, (it->second.flags & ORBHIP_MP_OBSERVED) != 0, kp.octave, kp.angle, motion, &q[i])) {
            memcpy(&qdesc[(size_t)i * 32], it->second.desc, 32);
            active++;
        }
    }
    for (size_t i = 0; i < S.kps.size(); i++) match[i] = -1;
    const int found = n_last ? search(S, u_right, occupied, q, qdesc, check_ori, th_high, match) : 0;
    if (queries_out) memcpy(queries_out, q.data(), q.size() * sizeof(orbo_proj_query));
    if (n_active) *n_active = active;
    if (nmatches) *nmatches = found;
    return ORBHIP_OK;
}

int orbhip_search_keyframe_points(orbhip_ctx *, uint64_t cur_key, uint64_t kf_set_key, uint64_t kf_row_key, const uint64_t *found_keys,
                                  int n_found, const orbhip_local_camera *cam, const uint8_t *occupied, int check_ori, int th_high,
                                  orbhip_proj_query *queries_out, int *n_active, int32_t *match, int *nmatches)
{
    if (!g.sets.count(cur_key) || !g.sets[cur_key].grid || (kf_set_key && !g.sets.count(kf_set_key)) || !g.rows.count(kf_row_key) ||
        cam->nlevels < 1 || cam->nlevels > 16)
        return ORBHIP_E_ARG;
    const Set &S = g.sets[cur_key];
    const std::vector<std::pair<uint64_t, unsigned> > &row = g.rows[kf_row_key];
    const int nq = (int)row.size();
    if (nq != (kf_set_key ? (int)g.sets[kf_set_key].kps.size() : 0)) return ORBHIP_E_ARG;
    const std::set<uint64_t> found(found_keys, found_keys + n_found);
    const refpt::Camera C = camera_of(cam);
    std::vector<orbo_proj_query> q(nq);
    std::vector<uint8_t> qdesc((size_t)nq * 32, 0);
    int active = 0;
    for (int i = 0; i < nq; i++) {
        memset(&q[i], 0, sizeof q[i]);
        auto it = g.points.find(row[i].first);
        if (!row[i].first || it == g.points.end() || g.incarnation[row[i].first] != row[i].second) continue;
        if ((it->second.flags & ORBHIP_MP_BAD) || found.count(row[i].first)) continue;
        if (refpt::kf_query(C, it->second.pos, it->second.mn, it->second.mx, g.sets[kf_set_key].kps[i].angle, &q[i])) {
            memcpy(&qdesc[(size_t)i * 32], it->second.desc, 32);
            active++;
        }
    }
    for (size_t i = 0; i < S.kps.size(); i++) match[i] = -1;
    const int n = nq ? search(S, NULL, occupied, q, qdesc, check_ori, th_high, match) : 0;
    if (queries_out) memcpy(queries_out, q.data(), q.size() * sizeof(orbo_proj_query));
    if (n_active) *n_active = active;
    if (nmatches) *nmatches = n;
    return ORBHIP_OK;
}

// linked by LocalMap.cc / LocalMapCollect.cc, never reached by these programs
int orbhip_search_local_points(orbhip_ctx *, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, const uint64_t *,
                               const uint8_t *, int, float, orbhip_local_point *, int *, int32_t *, int *)
{
    return unreachable("orbhip_search_local_points");
}
int orbhip_map_vote(orbhip_ctx *, int, const uint64_t *, uint64_t *, int32_t *, int, int *) { return unreachable("orbhip_map_vote"); }
int orbhip_map_collect(orbhip_ctx *, int, const uint64_t *, uint64_t *, int, int *) { return unreachable("orbhip_map_collect"); }
int orbhip_track_local_points(orbhip_ctx *, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, int, const uint64_t *, int,
                              const uint64_t *, float, uint64_t *, int, int *, orbhip_local_point *, int *, int32_t *, int *)
{
    return unreachable("orbhip_track_local_points");
}
}

// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (these programs link neither)
namespace ORB_SLAM2
{
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
}
