// mock_refresh.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch::RefreshPoints calls, for the programs that run it
// without a device (test_refresh_mock, test_refresh_mock_asan): the store keeps what orbhip_map_put was given, the sets keep
// keypoints and descriptors, orbhip_map_refresh is MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth restated over
// those copies (sorted rows for the median, the operations of docs/parity.md for the normal) with the library's argument checks,
// orbhip_map_get reads the store back.  The entry points the class links but these programs never reach fail loudly.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "orbhip.h"
#include "slamlite.h"

namespace
{
struct Point {
    float pos[3], nrm[3], mn, mx;
    uint8_t desc[32], flags;
};
struct Set {
    std::vector<orbhip_keypoint> kps;
    std::vector<uint8_t> desc;
};
struct Mock {
    int maxPoints = 0, setLimit = 4;
    unsigned long clock = 0;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, Set> sets;
    std::map<uint64_t, unsigned long> stamp;   // least recently used out, as the library's table
} g;

void touch(uint64_t key) { g.stamp[key] = ++g.clock; }
void evict_to(size_t n)
{
    while (g.sets.size() > n) {
        uint64_t oldest = 0;
        unsigned long t = ~0ul;
        for (auto &kv : g.sets)
            if (g.stamp[kv.first] < t) t = g.stamp[kv.first], oldest = kv.first;
        g.sets.erase(oldest);
        g.stamp.erase(oldest);
    }
}

int hamming(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

double norm3(const float d[3]) { return std::sqrt(((double)d[0] * d[0] + (double)d[1] * d[1]) + (double)d[2] * d[2]); }

int unreachable(const char *who)
{
    fprintf(stderr, "mock_refresh: %s is not modelled\n", who);
    return ORBHIP_E_ARG;
}
}  // namespace

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return (orbhip_ctx *)&g; }
void orbhip_destroy(orbhip_ctx *) {}
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g = Mock(); g.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *) { g.points.clear(); return ORBHIP_OK; }
int orbhip_set_limit(orbhip_ctx *, int n)
{
    g.setLimit = n < 4 ? 4 : n > 96 ? 96 : n;
    evict_to((size_t)g.setLimit);
    return g.setLimit;
}
int orbhip_set_drop(orbhip_ctx *, uint64_t key)
{
    if (key) g.sets.erase(key); else g.sets.clear();
    return ORBHIP_OK;
}
int orbhip_set_has(orbhip_ctx *, uint64_t key, int n) { return g.sets.count(key) && (int)g.sets[key].kps.size() == n; }
int orbhip_set_info(orbhip_ctx *, uint64_t key, int *n, int *ng, uint64_t *fp)
{
    if (!g.sets.count(key)) return 0;
    touch(key);
    if (n) *n = (int)g.sets[key].kps.size();
    if (ng) *ng = 0;
    if (fp) *fp = 0x9E3779B97F4A7C15ull ^ (uint64_t)g.sets[key].kps.size();   // (what orbhip_set_fingerprint_rows below gives)
    return 1;
}
uint64_t orbhip_set_fingerprint_rows(const orbhip_keypoint *, const uint8_t *, const uint8_t *, int n) { return 0x9E3779B97F4A7C15ull ^ (uint64_t)n; }
uint64_t orbhip_frame_fingerprint(const orbhip_ctx *) { return 0; }
int orbhip_set_put_from_frame(orbhip_ctx *, uint64_t, orbhip_ctx *, const int32_t *, const int32_t *, const int32_t *, int) { return unreachable("orbhip_set_put_from_frame"); }
int orbhip_set_put(orbhip_ctx *, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *, const int32_t *,
                   const int32_t *, int, float, float, float, float)
{
    if (!key || n <= 0) return ORBHIP_E_ARG;
    if (!g.sets.count(key)) evict_to((size_t)g.setLimit - 1);
    Set &S = g.sets[key];
    S.kps.assign(kps, kps + n);
    S.desc.assign(desc, desc + (size_t)n * 32);
    touch(key);
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
    for (int i = 0; i < n; i++) g.points.erase(keys[i]);
    return ORBHIP_OK;
}

int orbhip_map_refresh(orbhip_ctx *, const orbhip_refresh_params *prm, int nkf, const orbhip_refresh_kf *kfs, int P, const uint64_t *point_keys,
                       const int32_t *off, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *ref_pos, uint8_t *status,
                       int32_t *best_pos, uint8_t *desc_out, float *normal_out, float *min_dist_out, float *max_dist_out)
{
    if (!prm || nkf < 0 || P < 0) return ORBHIP_E_ARG;
    if (P == 0) return ORBHIP_OK;
    const bool wantDesc = prm->what & ORBHIP_REFRESH_DESC, wantNormal = prm->what & ORBHIP_REFRESH_NORMAL;
    if (prm->what < 1 || prm->what > 3 || prm->nlevels < 1 || prm->nlevels > 16 || off[0] != 0) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++)
        if (off[p + 1] < off[p]) return ORBHIP_E_ARG;
    for (int p = 0; p < P; p++)
        if (off[p + 1] - off[p] >= (1 << 20)) return ORBHIP_E_SIZE;
    std::set<uint64_t> seen, distinct;
    for (int p = 0; p < P; p++)
        if (!g.points.count(point_keys[p]) || !seen.insert(point_keys[p]).second) return ORBHIP_E_ARG;
    for (int k = 0; k < nkf; k++) distinct.insert(kfs[k].set_key);
    if ((int)distinct.size() > g.setLimit) return ORBHIP_E_ARG;
    for (int k = 0; k < nkf; k++) {
        if (!g.sets.count(kfs[k].set_key)) return ORBHIP_E_ARG;
        const Set &S = g.sets[kfs[k].set_key];
        for (size_t i = 0; i < S.kps.size(); i++)
            if (S.kps[i].octave < 0 || S.kps[i].octave >= prm->nlevels) return ORBHIP_E_ARG;
    }
    for (int j = 0; j < off[P]; j++)
        if (obs_kf[j] < 0 || obs_kf[j] >= nkf || obs_idx[j] < 0 || obs_idx[j] >= (int)g.sets[kfs[obs_kf[j]].set_key].kps.size()) return ORBHIP_E_ARG;
    for (int p = 0; p < P && wantNormal; p++)
        if (off[p + 1] > off[p] && (ref_pos[p] < 0 || ref_pos[p] >= off[p + 1] - off[p])) return ORBHIP_E_ARG;

    for (int p = 0; p < P; p++) {
        Point &Q = g.points[point_keys[p]];
        const int s = off[p], N = off[p + 1] - s;
        int st = 0, best = -1;
        if (!(Q.flags & ORBHIP_MP_BAD) && N > 0) {
            if (wantDesc) {   // ref: src/MapPoint.cc:257-322
                std::vector<int> rows;
                for (int j = 0; j < N; j++)
                    if (!(kfs[obs_kf[s + j]].flags & ORBHIP_KF_BAD)) rows.push_back(j);
                const size_t n = rows.size();
                int bestMedian = 0x7FFFFFFF;
                for (size_t i = 0; i < n; i++) {
                    const uint8_t *a = &g.sets[kfs[obs_kf[s + rows[i]]].set_key].desc[(size_t)obs_idx[s + rows[i]] * 32];
                    std::vector<int> v(n);
                    for (size_t j = 0; j < n; j++) v[j] = hamming(a, &g.sets[kfs[obs_kf[s + rows[j]]].set_key].desc[(size_t)obs_idx[s + rows[j]] * 32]);
                    std::sort(v.begin(), v.end());
                    const int median = v[(size_t)(0.5 * (n - 1))];
                    if (median < bestMedian) bestMedian = median, best = rows[i];
                }
                if (best >= 0) {
                    memcpy(Q.desc, &g.sets[kfs[obs_kf[s + best]].set_key].desc[(size_t)obs_idx[s + best] * 32], 32);
                    st |= ORBHIP_REFRESH_DESC;
                }
            }
            if (wantNormal) {   // ref: :345-386, docs/parity.md
                float normal[3] = {0.f, 0.f, 0.f};
                for (int j = 0; j < N; j++) {
                    const float *O = kfs[obs_kf[s + j]].Ow;
                    const float d[3] = {Q.pos[0] - O[0], Q.pos[1] - O[1], Q.pos[2] - O[2]};
                    const float a = (float)(1.0 / norm3(d));
                    for (int c = 0; c < 3; c++) {
                        const float t = d[c] * a;
                        normal[c] = t + normal[c];
                    }
                }
                const float inv = (float)(1.0 / (double)N);
                const int r = s + ref_pos[p];
                const float *O = kfs[obs_kf[r]].Ow;
                const float d[3] = {Q.pos[0] - O[0], Q.pos[1] - O[1], Q.pos[2] - O[2]};
                const float dist = (float)norm3(d);
                const int level = g.sets[kfs[obs_kf[r]].set_key].kps[obs_idx[r]].octave;
                Q.mx = dist * prm->scale_factors[level];
                Q.mn = Q.mx / prm->scale_factors[prm->nlevels - 1];
                for (int c = 0; c < 3; c++) Q.nrm[c] = normal[c] * inv;
                st |= ORBHIP_REFRESH_NORMAL;
            }
        }
        status[p] = (uint8_t)st;
        if (best_pos) best_pos[p] = best;
        if (desc_out) memcpy(desc_out + 32 * (size_t)p, Q.desc, 32);
        if (normal_out) memcpy(normal_out + 3 * (size_t)p, Q.nrm, 12);
        if (min_dist_out) min_dist_out[p] = Q.mn;
        if (max_dist_out) max_dist_out[p] = Q.mx;
    }
    return ORBHIP_OK;
}

int orbhip_map_get(orbhip_ctx *, int n, const uint64_t *keys, float *pos, float *normal, float *min_dist, float *max_dist, uint8_t *desc,
                   uint8_t *flags)
{
    for (int i = 0; i < n; i++)
        if (!g.points.count(keys[i])) return ORBHIP_E_ARG;
    for (int i = 0; i < n; i++) {
        const Point &Q = g.points[keys[i]];
        if (pos) memcpy(pos + 3 * (size_t)i, Q.pos, 12);
        if (normal) memcpy(normal + 3 * (size_t)i, Q.nrm, 12);
        if (min_dist) min_dist[i] = Q.mn;
        if (max_dist) max_dist[i] = Q.mx;
        if (desc) memcpy(desc + 32 * (size_t)i, Q.desc, 32);
        if (flags) flags[i] = Q.flags;
    }
    return ORBHIP_OK;
}

// linked by the other LocalMap*.cc files, never reached by these programs
int orbhip_map_kf_init(orbhip_ctx *, int, int) { return unreachable("orbhip_map_kf_init"); }
int orbhip_map_kf_clear(orbhip_ctx *) { return unreachable("orbhip_map_kf_clear"); }
int orbhip_map_kf_put(orbhip_ctx *, uint64_t, int, const uint64_t *) { return unreachable("orbhip_map_kf_put"); }
int orbhip_map_kf_set(orbhip_ctx *, uint64_t, int, const int32_t *, const uint64_t *) { return unreachable("orbhip_map_kf_set"); }
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t) { return unreachable("orbhip_map_kf_erase"); }
int orbhip_fuse_row(orbhip_ctx *, uint64_t, const orbhip_fuse_target *, int, const uint8_t *, const float *, orbhip_proj_query *, int32_t *,
                    int32_t *, int32_t *)
{
    return unreachable("orbhip_fuse_row");
}
int orbhip_map_collect(orbhip_ctx *, int, const uint64_t *, uint64_t *, int, int *) { return unreachable("orbhip_map_collect"); }
int orbhip_fuse_collect(orbhip_ctx *, const orbhip_fuse_target *, uint64_t, int, const uint64_t *, const float *, uint64_t *, int, int *,
                        orbhip_proj_query *, int32_t *, int32_t *, int32_t *)
{
    return unreachable("orbhip_fuse_collect");
}
int orbhip_window_best_set(orbhip_ctx *, uint64_t, const float *, const float *, int, const orbhip_proj_query *, const uint8_t *, int,
                           int32_t *, int32_t *)
{
    return unreachable("orbhip_window_best_set");
}
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
