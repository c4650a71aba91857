// mock_collect.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch calls for UpdateLocalMap (no device, no
// liborbhip): points by key with a serial number per put of a new key, key-frame rows of (key, serial) entries that resolve only
// while the point with that serial is in the store.  The searches are stubs: this program tests the bookkeeping.
#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "orbhip.h"
#include "slamlite.h"

namespace
{
struct Point { uint8_t flags; uint64_t serial; };
struct Mock {
    int maxPoints = 0, maxKfs = 0, maxRow = 0;
    uint64_t nextSerial = 1;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, std::vector<std::pair<uint64_t, uint64_t> > > rows;
    const Point *resolve(const std::pair<uint64_t, uint64_t> &e) const
    {
        if (!e.first) return nullptr;
        std::map<uint64_t, Point>::const_iterator it = points.find(e.first);
        if (it == points.end() || it->second.serial != e.second || (it->second.flags & ORBHIP_MP_BAD)) return nullptr;
        return &it->second;
    }
} g;
}  // namespace

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return (orbhip_ctx *)&g; }
void orbhip_destroy(orbhip_ctx *) {}
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g = Mock(); g.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *) { g.points.clear(); return ORBHIP_OK; }
int orbhip_set_limit(orbhip_ctx *, int n) { return n; }
int orbhip_set_drop(orbhip_ctx *, uint64_t) { return ORBHIP_OK; }
int orbhip_set_has(orbhip_ctx *, uint64_t, int) { return 1; }
int orbhip_set_put(orbhip_ctx *, uint64_t, const orbhip_keypoint *, const uint8_t *, int, const int32_t *, const int32_t *, const int32_t *,
                   int, float, float, float, float) { return ORBHIP_OK; }
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *, const float *, const float *, const float *, const uint8_t *,
                   const uint8_t *flags)
{
    for (int i = 0; i < n; i++) {
        std::map<uint64_t, Point>::iterator it = g.points.find(keys[i]);
        if (it != g.points.end()) { it->second.flags = flags[i]; continue; }
        if ((int)g.points.size() >= g.maxPoints) return ORBHIP_E_CAPACITY;
        Point p = {flags[i], g.nextSerial++};
        g.points[keys[i]] = p;
    }
    return ORBHIP_OK;
}
int orbhip_map_update_flags(orbhip_ctx *, int n, const uint64_t *keys, const uint8_t *flags)
{
    for (int i = 0; i < n; i++) {
        if (!g.points.count(keys[i])) return ORBHIP_E_ARG;
        g.points[keys[i]].flags = flags[i];
    }
    return ORBHIP_OK;
}
int orbhip_map_erase(orbhip_ctx *, int n, const uint64_t *keys)
{
    for (int i = 0; i < n; i++) g.points.erase(keys[i]);
    return ORBHIP_OK;
}
int orbhip_search_local_points(orbhip_ctx *, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, const uint64_t *,
                               const uint8_t *, int nq, float, orbhip_local_point *points, int *n_to_match, int32_t *, int *nmatches)
{
    memset(points, 0, sizeof(orbhip_local_point) * nq);
    *n_to_match = *nmatches = 0;
    return ORBHIP_OK;
}
int orbhip_map_kf_init(orbhip_ctx *, int max_kfs, int max_row) { g.maxKfs = max_kfs, g.maxRow = max_row; g.rows.clear(); return ORBHIP_OK; }
int orbhip_map_kf_clear(orbhip_ctx *) { g.rows.clear(); return ORBHIP_OK; }
int orbhip_map_kf_put(orbhip_ctx *, uint64_t kf_key, int n, const uint64_t *point_keys)
{
    if (!kf_key || n > g.maxRow) return ORBHIP_E_ARG;
    std::vector<std::pair<uint64_t, uint64_t> > row(n);
    std::set<uint64_t> in;
    for (int i = 0; i < n; i++) {
        if (!point_keys[i]) continue;
        if (!g.points.count(point_keys[i]) || !in.insert(point_keys[i]).second) return ORBHIP_E_ARG;
        row[i] = std::make_pair(point_keys[i], g.points[point_keys[i]].serial);
    }
    if (!g.rows.count(kf_key) && (int)g.rows.size() >= g.maxKfs) return ORBHIP_E_CAPACITY;
    g.rows[kf_key] = row;
    return ORBHIP_OK;
}
int orbhip_map_kf_set(orbhip_ctx *, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys)
{
    if (!g.rows.count(kf_key)) return ORBHIP_E_ARG;
    std::vector<std::pair<uint64_t, uint64_t> > row = g.rows[kf_key];
    for (int j = 0; j < m; j++) {
        if (idx[j] < 0 || idx[j] >= (int)row.size()) return ORBHIP_E_ARG;
        if (point_keys[j] && !g.points.count(point_keys[j])) return ORBHIP_E_ARG;
        row[idx[j]] = point_keys[j] ? std::make_pair(point_keys[j], g.points[point_keys[j]].serial) : std::make_pair((uint64_t)0, (uint64_t)0);
    }
    for (int j = 0; j < m; j++)
        for (size_t i = 0; i < row.size(); i++)
            if (row[idx[j]].first && row[i] == row[idx[j]] && (int)i != idx[j]) return ORBHIP_E_ARG;
    g.rows[kf_key] = row;
    return ORBHIP_OK;
}
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t kf_key) { g.rows.erase(kf_key); return ORBHIP_OK; }
int orbhip_map_vote(orbhip_ctx *, int n, const uint64_t *frame_point_keys, uint64_t *kf_keys_out, int32_t *counts_out, int cap, int *nout)
{
    std::map<uint64_t, int> marks;
    for (int i = 0; i < n; i++)
        if (frame_point_keys[i]) marks[frame_point_keys[i]]++;
    int k = 0;
    for (std::map<uint64_t, std::vector<std::pair<uint64_t, uint64_t> > >::const_iterator r = g.rows.begin(); r != g.rows.end(); ++r) {
        int sum = 0;
        for (size_t i = 0; i < r->second.size(); i++)
            if (g.resolve(r->second[i]) && marks.count(r->second[i].first)) sum += marks[r->second[i].first];
        if (!sum) continue;
        if (k < cap) kf_keys_out[k] = r->first, counts_out[k] = sum;
        k++;
    }
    *nout = k;
    return k > cap ? ORBHIP_E_CAPACITY : ORBHIP_OK;
}
int orbhip_map_collect(orbhip_ctx *, int nkf, const uint64_t *kf_keys, uint64_t *local_keys_out, int cap, int *nlocal)
{
    std::set<uint64_t> taken;
    int k = 0;
    for (int f = 0; f < nkf; f++) {
        if (!g.rows.count(kf_keys[f])) return ORBHIP_E_ARG;
        const std::vector<std::pair<uint64_t, uint64_t> > &row = g.rows[kf_keys[f]];
        for (size_t i = 0; i < row.size(); i++) {
            if (!g.resolve(row[i]) || !taken.insert(row[i].first).second) continue;
            if (k < cap) local_keys_out[k] = row[i].first;
            k++;
        }
    }
    *nlocal = k;
    return k > cap ? ORBHIP_E_CAPACITY : ORBHIP_OK;
}
int orbhip_track_local_points(orbhip_ctx *c, uint64_t, const float *, const uint8_t *, const orbhip_local_camera *, int nkf,
                              const uint64_t *kf_keys, int, const uint64_t *, float, uint64_t *local_keys_out, int cap, int *nlocal,
                              orbhip_local_point *points, int *n_to_match, int32_t *, int *nmatches)
{
    const int rc = orbhip_map_collect(c, nkf, kf_keys, local_keys_out, cap, nlocal);
    if (rc) return rc;
    memset(points, 0, sizeof(orbhip_local_point) * *nlocal);
    *n_to_match = *nmatches = 0;
    return ORBHIP_OK;
}
}

// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (this program links neither)
namespace ORB_SLAM2
{
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
}
