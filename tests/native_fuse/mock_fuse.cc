// mock_fuse.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch calls, for the programs that run FuseInTargets and
// FuseCandidates without a device (test_fuse_mock, test_fuse_mock_asan): the store keeps what orbhip_map_put was given, the
// key-frame table keeps keys with the point's incarnation (an erased point's entries never resolve again, as the device's
// generation count has it), the sets keep keypoints and descriptors, orbhip_fuse_row / orbhip_fuse_collect are the projection of
// ref_fuse.h over those copies with the oracle's window search behind it.  The entry points the class links but these programs
// never reach (vote, the local-points and projection searches) fail loudly.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "orbhip.h"
#include "ref_fuse.h"

namespace
{
struct Point {
    float pos[3], nrm[3], mn, mx;
    uint8_t desc[32], flags;
};
struct Set {
    std::vector<orbhip_keypoint> kps;
    std::vector<uint8_t> desc;
    float gp[4];
    bool grid;
};
typedef std::vector<std::pair<uint64_t, unsigned> > Row;   // (point key, incarnation at the time)
struct Mock {
    int maxPoints = 0, maxKfs = 0, maxRow = 0, setLimit = 4;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, unsigned> incarnation;                              // key -> how often it was erased
    std::map<uint64_t, Set> sets;
    std::map<uint64_t, Row> rows;
} g;

reffuse::Camera camera_of(const orbhip_local_camera *c)
{
    reffuse::Camera C;
    memset(&C, 0, sizeof C);
    memcpy(C.R, c->Rcw, sizeof C.R), memcpy(C.t, c->tcw, sizeof C.t), memcpy(C.Ow, c->Ow, sizeof C.Ow);
    C.fx = c->fx, C.fy = c->fy, C.cx = c->cx, C.cy = c->cy, C.mbf = c->mbf;
    C.minX = c->min_x, C.maxX = c->max_x, C.minY = c->min_y, C.maxY = c->max_y;
    memcpy(C.sf, c->scale_factors, sizeof C.sf);
    C.logS = c->log_scale_factor, C.th = c->th, C.nlevels = c->nlevels;
    return C;
}

// the point a row entry names now, or NULL: empty, erased, erased and put again, bad
const Point *resolve(const std::pair<uint64_t, unsigned> &e)
{
    if (!e.first) return NULL;
    auto it = g.points.find(e.first);
    if (it == g.points.end() || g.incarnation[e.first] != e.second || (it->second.flags & ORBHIP_MP_BAD)) return NULL;
    return &it->second;
}

bool target_ok(const orbhip_fuse_target &t)
{
    return g.sets.count(t.set_key) && g.sets[t.set_key].grid && t.cam.nlevels >= 1 && t.cam.nlevels <= 16 && std::isfinite(t.cam.th);
}

// queries of the points `pts` (NULL: inactive) in one target, then the oracle's gated window search
int project_and_search(const orbhip_fuse_target &t, const std::vector<const Point *> &pts, const float *u_right, orbhip_proj_query *queries_out,
                       int32_t *best_idx, int32_t *best_dist)
{
    const Set &S = g.sets[t.set_key];
    const reffuse::Camera C = camera_of(&t.cam);
    const int n = (int)pts.size();
    std::vector<orbo_proj_query> q(n);
    std::vector<uint8_t> qdesc((size_t)n * 32, 0);
    int active = 0;
    for (int i = 0; i < n; i++) {
        memset(&q[i], 0, sizeof q[i]);
        if (!pts[i]) continue;
        if (reffuse::fuse_query(C, pts[i]->pos, pts[i]->nrm, pts[i]->mn, pts[i]->mx, &q[i])) {
            memcpy(&qdesc[(size_t)i * 32], pts[i]->desc, 32);
            active++;
        }
    }
    if (n)
        orbo_window_best(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), (int)S.kps.size(), u_right, t.inv_level_sigma2,
                         S.gp[0], S.gp[1], S.gp[2], S.gp[3], q.data(), qdesc.data(), n, best_idx, best_dist);
    if (queries_out) memcpy(queries_out, q.data(), q.size() * sizeof(orbo_proj_query));
    return active;
}

int unreachable(const char *who)
{
    fprintf(stderr, "mock_fuse: %s is not modelled\n", who);
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
int orbhip_set_limit(orbhip_ctx *, int n) { return g.setLimit = n < 4 ? 4 : n > 96 ? 96 : n; }
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
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *pos, const float *nrm, const float *mn, const float *mx,
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
        memcpy(P.pos, pos + 3 * i, 12), memcpy(P.nrm, nrm + 3 * i, 12);
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
    Row row(n);
    std::set<uint64_t> seen;
    for (int i = 0; i < n; i++) {
        if (point_keys[i] && (!g.points.count(point_keys[i]) || !seen.insert(point_keys[i]).second)) return ORBHIP_E_ARG;
        row[i] = std::make_pair(point_keys[i], point_keys[i] ? g.incarnation[point_keys[i]] : 0u);
    }
    g.rows[kf_key] = row;
    return ORBHIP_OK;
}
int orbhip_map_kf_set(orbhip_ctx *, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys)
{
    if (!g.rows.count(kf_key)) return ORBHIP_E_ARG;
    Row row = g.rows[kf_key];
    for (int j = 0; j < m; j++) {
        if (idx[j] < 0 || idx[j] >= (int)row.size() || (point_keys[j] && !g.points.count(point_keys[j]))) return ORBHIP_E_ARG;
        row[idx[j]] = std::make_pair(point_keys[j], point_keys[j] ? g.incarnation[point_keys[j]] : 0u);
    }
    std::set<uint64_t> seen;                      // a point twice in the row as it will be: refused, as the library does
    for (size_t i = 0; i < row.size(); i++)
        if (row[i].first && !seen.insert(row[i].first).second) return ORBHIP_E_ARG;
    g.rows[kf_key] = row;
    return ORBHIP_OK;
}
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t kf_key) { g.rows.erase(kf_key); return ORBHIP_OK; }

int orbhip_fuse_row(orbhip_ctx *, uint64_t src_row_key, const orbhip_fuse_target *targets, int K, const uint8_t *skip, const float *u_right,
                    orbhip_proj_query *queries_out, int32_t *best_idx, int32_t *best_dist, int32_t *n_active)
{
    if (K < 0) return ORBHIP_E_ARG;
    if (K == 0) return ORBHIP_OK;
    if (!g.rows.count(src_row_key)) return ORBHIP_E_ARG;
    std::set<uint64_t> distinct;
    for (int k = 0; k < K; k++) {
        if (!target_ok(targets[k])) return ORBHIP_E_ARG;
        distinct.insert(targets[k].set_key);
    }
    if ((int)distinct.size() > g.setLimit) return ORBHIP_E_ARG;
    const Row &row = g.rows[src_row_key];
    const int n = (int)row.size();
    size_t urAt = 0;
    for (int k = 0; k < K; k++) {
        std::vector<const Point *> pts(n);
        for (int i = 0; i < n; i++) pts[i] = (skip && skip[(size_t)k * n + i]) ? NULL : resolve(row[i]);
        n_active[k] = project_and_search(targets[k], pts, u_right ? u_right + urAt : NULL, queries_out ? queries_out + (size_t)k * n : NULL,
                                         best_idx + (size_t)k * n, best_dist + (size_t)k * n);
        urAt += g.sets[targets[k].set_key].kps.size();
    }
    return ORBHIP_OK;
}

int orbhip_map_collect(orbhip_ctx *, int nkf, const uint64_t *kf_keys, uint64_t *local_keys_out, int cap, int *nlocal)
{
    std::set<uint64_t> seen;
    int n = 0;
    for (int k = 0; k < nkf; k++) {
        if (!g.rows.count(kf_keys[k])) return ORBHIP_E_ARG;
        const Row &row = g.rows[kf_keys[k]];
        for (size_t i = 0; i < row.size(); i++) {
            if (!resolve(row[i]) || !seen.insert(row[i].first).second) continue;
            if (n < cap) local_keys_out[n] = row[i].first;
            n++;
        }
    }
    *nlocal = n;
    return n > cap ? ORBHIP_E_CAPACITY : ORBHIP_OK;
}

int orbhip_fuse_collect(orbhip_ctx *c, const orbhip_fuse_target *target, uint64_t cur_row_key, int nkf, const uint64_t *kf_keys,
                        const float *u_right, uint64_t *keys_out, int cap, int *ncand, orbhip_proj_query *queries_out, int32_t *best_idx,
                        int32_t *best_dist, int32_t *n_active)
{
    if (!g.rows.count(cur_row_key) || !target_ok(*target)) return ORBHIP_E_ARG;
    for (int k = 0; k < nkf; k++)
        if (!g.rows.count(kf_keys[k])) return ORBHIP_E_ARG;
    std::vector<uint64_t> keys(cap > 0 ? cap : 1);
    int n = 0;
    const int rc = orbhip_map_collect(c, nkf, kf_keys, keys.data(), cap, &n);
    *ncand = n, *n_active = 0;
    for (int i = 0; i < n && i < cap; i++) keys_out[i] = keys[i];
    if (rc != ORBHIP_OK) return rc;
    std::set<uint64_t> held;                      // IsInKeyFrame: what the current key frame's row resolves to
    const Row &own = g.rows[cur_row_key];
    for (size_t i = 0; i < own.size(); i++)
        if (own[i].first && g.points.count(own[i].first) && g.incarnation[own[i].first] == own[i].second) held.insert(own[i].first);
    std::vector<const Point *> pts(n);
    for (int i = 0; i < n; i++) pts[i] = held.count(keys[i]) ? NULL : &g.points[keys[i]];
    *n_active = project_and_search(*target, pts, u_right, queries_out, best_idx, best_dist);
    return ORBHIP_OK;
}

int orbhip_window_best_set(orbhip_ctx *, uint64_t key, const float *u_right, const float *inv_level_sigma2, int nlevels,
                           const orbhip_proj_query *queries, const uint8_t *qdesc, int nq, int32_t *best_idx, int32_t *best_dist)
{
    if (!g.sets.count(key) || !g.sets[key].grid || (inv_level_sigma2 && (nlevels <= 0 || nlevels > 16))) return ORBHIP_E_ARG;
    const Set &S = g.sets[key];
    float sig[16] = {0};
    for (int l = 0; inv_level_sigma2 && l < nlevels; l++) sig[l] = inv_level_sigma2[l];
    orbo_window_best(reinterpret_cast<const orbo_keypoint *>(S.kps.data()), S.desc.data(), (int)S.kps.size(), u_right,
                     inv_level_sigma2 ? sig : NULL, S.gp[0], S.gp[1], S.gp[2], S.gp[3], reinterpret_cast<const orbo_proj_query *>(queries), qdesc,
                     nq, best_idx, best_dist);
    return ORBHIP_OK;
}

// linked by the other LocalMap*.cc files, never reached by these programs
int orbhip_search_local_points(orbhip_ctx *, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, const uint64_t *,
                               const uint8_t *, int, float, orbhip_local_point *, int *, int32_t *, int *)
{
    return unreachable("orbhip_search_local_points");
}
int orbhip_map_vote(orbhip_ctx *, int, const uint64_t *, uint64_t *, int32_t *, int, int *) { return unreachable("orbhip_map_vote"); }
int orbhip_track_local_points(orbhip_ctx *, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, int, const uint64_t *, int,
                              const uint64_t *, float, uint64_t *, int, int *, orbhip_local_point *, int *, int32_t *, int *)
{
    return unreachable("orbhip_track_local_points");
}
int orbhip_search_last_frame(orbhip_ctx *, uint64_t, uint64_t, const uint64_t *, int, const orbhip_local_camera *, int, const float *,
                             const uint8_t *, int, int, orbhip_proj_query *, int *, int32_t *, int *)
{
    return unreachable("orbhip_search_last_frame");
}
int orbhip_search_keyframe_points(orbhip_ctx *, uint64_t, uint64_t, uint64_t, const uint64_t *, int, const orbhip_local_camera *,
                                  const uint8_t *, int, int, orbhip_proj_query *, int *, int32_t *, int *)
{
    return unreachable("orbhip_search_keyframe_points");
}
}

// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (these programs link neither)
namespace ORB_SLAM2
{
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
}
