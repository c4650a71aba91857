// mock_ba.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch::BuildLocalBA / BuildBAProblem call, for the programs that
// run them without a device (test_baproblem_mock, test_baproblem_mock_asan).  The store keeps a flag byte and an incarnation number
// per point key, a key-frame row keeps (point key, incarnation) per entry, so that an entry whose point was erased or put again
// resolves to nothing -- what the slot and its generation do in the library.  orbhip_map_ba_problem is written from the header's
// definitions: the ordered union of the local rows, for every point its holders over all rows in ascending key, the fixed key
// frames by first appearance, the library's argument checks and its rule for too little room.  mock_ba_fail(1) makes it fail as a
// device error would; mock_ba_calls() counts its calls.  The entry points the class links but these programs never reach fail loudly.
#include <algorithm>
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
    uint8_t flags;
    unsigned long born;
};
typedef std::pair<uint64_t, unsigned long> Entry;   // point key (0: none), incarnation
struct Mock {
    int maxPoints = 0, maxKfs = 0, maxRow = 0;
    bool table = false;
    unsigned long clock = 0;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, std::vector<Entry> > rows;
} g;
bool g_fail = false;
long g_calls = 0;

bool resolves(const Entry &e)
{
    if (!e.first) return false;
    std::map<uint64_t, Point>::const_iterator it = g.points.find(e.first);
    return it != g.points.end() && it->second.born == e.second && !(it->second.flags & ORBHIP_MP_BAD);
}

bool entry_of(uint64_t key, Entry *e)
{
    if (!key) return *e = Entry(0, 0), true;
    std::map<uint64_t, Point>::const_iterator it = g.points.find(key);
    if (it == g.points.end()) return false;
    return *e = Entry(key, it->second.born), true;
}

bool twice(const std::vector<Entry> &row)
{
    std::set<uint64_t> seen;
    for (size_t i = 0; i < row.size(); i++)
        if (row[i].first && !seen.insert(row[i].first).second) return true;
    return false;
}

int unreachable(const char *who)
{
    fprintf(stderr, "mock_ba: %s is not modelled\n", who);
    return ORBHIP_E_ARG;
}
}  // namespace

void mock_ba_fail(int on) { g_fail = on != 0; }
long mock_ba_calls() { return g_calls; }

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return (orbhip_ctx *)&g; }
void orbhip_destroy(orbhip_ctx *) {}
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g = Mock(); g.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *) { g.points.clear(); return ORBHIP_OK; }
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *, const float *, const float *, const float *, const uint8_t *,
                   const uint8_t *flags)
{
    std::set<uint64_t> seen;
    size_t fresh = 0;
    for (int i = 0; i < n; i++) {
        if (!keys[i] || !seen.insert(keys[i]).second) return ORBHIP_E_ARG;
        fresh += g.points.count(keys[i]) ? 0 : 1;
    }
    if (g.points.size() + fresh > (size_t)g.maxPoints) return ORBHIP_E_CAPACITY;
    for (int i = 0; i < n; i++) {
        if (!g.points.count(keys[i])) g.points[keys[i]].born = ++g.clock;   // (an update keeps the slot and its generation)
        g.points[keys[i]].flags = flags[i];
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
int orbhip_map_kf_init(orbhip_ctx *, int max_kfs, int max_row)
{
    if (max_kfs <= 0 || max_row <= 0) return ORBHIP_E_ARG;
    g.rows.clear();
    g.maxKfs = max_kfs, g.maxRow = max_row, g.table = true;
    return ORBHIP_OK;
}
int orbhip_map_kf_clear(orbhip_ctx *) { g.rows.clear(); return ORBHIP_OK; }
int orbhip_map_kf_put(orbhip_ctx *, uint64_t kf_key, int n, const uint64_t *point_keys)
{
    if (!g.table || !kf_key || n < 0 || n > g.maxRow) return ORBHIP_E_ARG;
    std::vector<Entry> row(n);
    for (int i = 0; i < n; i++)
        if (!entry_of(point_keys[i], &row[i])) return ORBHIP_E_ARG;
    if (twice(row)) return ORBHIP_E_ARG;
    if (!g.rows.count(kf_key) && (int)g.rows.size() >= g.maxKfs) return ORBHIP_E_CAPACITY;
    g.rows[kf_key].swap(row);
    return ORBHIP_OK;
}
int orbhip_map_kf_set(orbhip_ctx *, uint64_t kf_key, int m, const int32_t *idx, const uint64_t *point_keys)
{
    if (!g.table || !g.rows.count(kf_key) || m < 0) return ORBHIP_E_ARG;
    std::vector<Entry> row = g.rows[kf_key];
    for (int j = 0; j < m; j++) {
        if (idx[j] < 0 || idx[j] >= (int)row.size()) return ORBHIP_E_ARG;
        if (!entry_of(point_keys[j], &row[idx[j]])) return ORBHIP_E_ARG;
    }
    if (twice(row)) return ORBHIP_E_ARG;
    g.rows[kf_key].swap(row);
    return ORBHIP_OK;
}
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t kf_key) { g.rows.erase(kf_key); return ORBHIP_OK; }

int orbhip_map_ba_problem(orbhip_ctx *, int nkf, const uint64_t *kf_keys, uint64_t *point_keys_out, int cap_points, int *npoints,
                          int32_t *edge_off_out, orbhip_ba_edge *edges_out, int cap_edges, int *nedges, uint64_t *fixed_keys_out,
                          int cap_fixed, int *nfixed)
{
    g_calls++;
    if (nkf < 0 || nkf > 65536 || cap_points < 0 || cap_edges < 0 || cap_fixed < 0 || !g.table) return ORBHIP_E_ARG;
    for (int k = 0; k < nkf; k++)
        if (!g.rows.count(kf_keys[k])) return ORBHIP_E_ARG;
    if (g_fail) return ORBHIP_E_HIP;
    // the ordered union of the local rows; the place of every local key (its first occurrence)
    std::vector<uint64_t> points;
    std::set<uint64_t> taken;
    std::map<uint64_t, int> local;
    for (int k = 0; k < nkf; k++) {
        if (!local.count(kf_keys[k])) local[kf_keys[k]] = k;
        const std::vector<Entry> &row = g.rows[kf_keys[k]];
        for (size_t i = 0; i < row.size(); i++)
            if (resolves(row[i]) && taken.insert(row[i].first).second) points.push_back(row[i].first);
    }
    // who holds each point, and at which feature, over all rows in ascending key
    std::map<uint64_t, std::vector<std::pair<uint64_t, size_t> > > holders;
    for (std::map<uint64_t, std::vector<Entry> >::const_iterator r = g.rows.begin(); r != g.rows.end(); ++r)
        for (size_t i = 0; i < r->second.size(); i++)
            if (resolves(r->second[i]) && taken.count(r->second[i].first)) holders[r->second[i].first].push_back(std::make_pair(r->first, i));
    std::vector<uint64_t> fixed;
    std::map<uint64_t, int> fixedAt;
    std::vector<orbhip_ba_edge> edges;
    std::vector<int32_t> off(1, 0);
    for (size_t j = 0; j < points.size(); j++) {
        const std::vector<std::pair<uint64_t, size_t> > &h = holders[points[j]];
        for (size_t m = 0; m < h.size(); m++) {
            orbhip_ba_edge e;
            if (local.count(h[m].first)) {
                e.kf = local[h[m].first];
            } else {
                if (!fixedAt.count(h[m].first)) {
                    fixedAt[h[m].first] = (int)fixed.size();
                    fixed.push_back(h[m].first);
                }
                e.kf = nkf + fixedAt[h[m].first];
            }
            e.idx = (int32_t)h[m].second;
            edges.push_back(e);
        }
        off.push_back((int32_t)edges.size());
    }
    *npoints = (int)points.size(), *nedges = (int)edges.size(), *nfixed = (int)fixed.size();
    if (*npoints > cap_points || *nedges > cap_edges || *nfixed > cap_fixed) return ORBHIP_E_CAPACITY;
    std::copy(points.begin(), points.end(), point_keys_out);
    std::copy(off.begin(), off.end(), edge_off_out);
    std::copy(edges.begin(), edges.end(), edges_out);
    std::copy(fixed.begin(), fixed.end(), fixed_keys_out);
    return ORBHIP_OK;
}

// linked by LocalMap.cc and LocalMapCollect.cc, never reached by these programs
int orbhip_set_limit(orbhip_ctx *, int n) { return n < 4 ? 4 : n > 96 ? 96 : n; }   // (no sets in these programs)
int orbhip_set_drop(orbhip_ctx *, uint64_t) { return ORBHIP_OK; }
int orbhip_set_has(orbhip_ctx *, uint64_t, int) { return unreachable("orbhip_set_has"), 0; }
int orbhip_set_put(orbhip_ctx *, uint64_t, const orbhip_keypoint *, const uint8_t *, int, const int32_t *, const int32_t *, const int32_t *, int,
                   float, float, float, float)
{
    return unreachable("orbhip_set_put");
}
int orbhip_map_collect(orbhip_ctx *, int, const uint64_t *, uint64_t *, int, int *) { return unreachable("orbhip_map_collect"); }
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
}

// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (these programs link neither)
namespace ORB_SLAM2
{
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;
}
