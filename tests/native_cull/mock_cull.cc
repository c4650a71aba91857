// mock_cull.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch::CullCounts / KeyFrameCulled call, for the programs that
// run them without a device (test_cull_mock, test_cull_mock_asan).  The store keeps a flag byte and an incarnation number per point
// key, a key-frame row keeps (point key, incarnation) per entry, so that an entry whose point was erased or put again resolves to
// nothing -- what the slot and its generation do in the library.  Levels are a byte vector per row with the library's lifetime.
// orbhip_map_cull counts by walking, for every resolving entry of the candidate's row, the other rows that hold the same point, with
// the header's definitions and the library's argument checks.  The entry points the class links but these programs never reach fail
// loudly.
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
    std::map<uint64_t, std::vector<uint8_t> > levels;
} g;

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

bool levels_current(uint64_t kf)
{
    std::map<uint64_t, std::vector<uint8_t> >::const_iterator it = g.levels.find(kf);
    return it != g.levels.end() && it->second.size() >= g.rows[kf].size();
}

int unreachable(const char *who)
{
    fprintf(stderr, "mock_cull: %s is not modelled\n", who);
    return ORBHIP_E_ARG;
}
}  // namespace

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
    g.rows.clear(), g.levels.clear();
    g.maxKfs = max_kfs, g.maxRow = max_row, g.table = true;
    return ORBHIP_OK;
}
int orbhip_map_kf_clear(orbhip_ctx *) { g.rows.clear(), g.levels.clear(); return ORBHIP_OK; }
int orbhip_map_kf_put(orbhip_ctx *, uint64_t kf_key, int n, const uint64_t *point_keys)
{
    if (!g.table || !kf_key || n < 0 || n > g.maxRow) return ORBHIP_E_ARG;
    std::vector<Entry> row(n);
    for (int i = 0; i < n; i++)
        if (!entry_of(point_keys[i], &row[i])) return ORBHIP_E_ARG;
    if (twice(row)) return ORBHIP_E_ARG;
    if (!g.rows.count(kf_key) && (int)g.rows.size() >= g.maxKfs) return ORBHIP_E_CAPACITY;
    g.rows[kf_key].swap(row);   // (a known key keeps its levels)
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
int orbhip_map_kf_erase(orbhip_ctx *, uint64_t kf_key) { g.rows.erase(kf_key), g.levels.erase(kf_key); return ORBHIP_OK; }

int orbhip_map_kf_levels(orbhip_ctx *, int m, const uint64_t *kf_keys, const int32_t *off, const uint8_t *bytes)
{
    if (!g.table || m < 0) return ORBHIP_E_ARG;
    if (m == 0) return ORBHIP_OK;
    if (off[0] != 0) return ORBHIP_E_ARG;
    std::set<uint64_t> seen;
    for (int q = 0; q < m; q++)
        if (!g.rows.count(kf_keys[q]) || !seen.insert(kf_keys[q]).second || off[q + 1] < off[q] || off[q + 1] - off[q] > g.maxRow) return ORBHIP_E_ARG;
    for (int i = 0; i < off[m]; i++)
        if (bytes[i] & 0x30) return ORBHIP_E_ARG;
    for (int q = 0; q < m; q++) g.levels[kf_keys[q]].assign(bytes + off[q], bytes + off[q + 1]);
    return ORBHIP_OK;
}
int orbhip_map_kf_levels_missing(orbhip_ctx *, uint64_t *kf_keys_out, int cap, int *nout)
{
    int n = 0;
    for (std::map<uint64_t, std::vector<Entry> >::const_iterator r = g.rows.begin(); r != g.rows.end(); ++r)   // (ascending keys)
        if (!levels_current(r->first)) {
            if (n < cap) kf_keys_out[n] = r->first;
            n++;
        }
    *nout = n;
    return n > cap ? ORBHIP_E_CAPACITY : ORBHIP_OK;
}

int orbhip_map_cull(orbhip_ctx *, int K, const uint64_t *kf_keys, int monocular, int th_obs, orbhip_cull_count *counts, uint8_t *redundant,
                    uint8_t *entry_state)
{
    if (K < 0 || K > 65536 || th_obs < 1 || !g.table) return ORBHIP_E_ARG;
    if (K == 0) return ORBHIP_OK;
    for (int k = 0; k < K; k++)
        if (!g.rows.count(kf_keys[k])) return ORBHIP_E_ARG;
    for (std::map<uint64_t, std::vector<Entry> >::const_iterator r = g.rows.begin(); r != g.rows.end(); ++r)
        if (!levels_current(r->first)) return ORBHIP_E_ARG;
    // who holds each point, and at which feature: the point's observation map (ref: src/LocalMapping.cc:2730)
    std::map<uint64_t, std::vector<std::pair<uint64_t, size_t> > > holders;
    for (std::map<uint64_t, std::vector<Entry> >::const_iterator r = g.rows.begin(); r != g.rows.end(); ++r)
        for (size_t i = 0; i < r->second.size(); i++)
            if (resolves(r->second[i])) holders[r->second[i].first].push_back(std::make_pair(r->first, i));
    for (int k = 0; k < K; k++) {
        const std::vector<Entry> &row = g.rows[kf_keys[k]];
        const std::vector<uint8_t> &lv = g.levels[kf_keys[k]];
        int nMPs = 0, nRed = 0;
        if (entry_state) memset(entry_state + (size_t)k * g.maxRow, 0, g.maxRow);
        for (size_t i = 0; i < row.size(); i++) {
            if (!resolves(row[i])) continue;
            if (!monocular && (lv[i] & 0x80)) continue;
            nMPs++;
            const std::vector<std::pair<uint64_t, size_t> > &h = holders[row[i].first];
            int obs = 0, others = 0;
            for (size_t j = 0; j < h.size(); j++) {
                const uint8_t b = g.levels[h[j].first][h[j].second];
                obs += 1 + ((b >> 6) & 1);
                if (h[j].first != kf_keys[k] && (b & 15) <= (lv[i] & 15) + 1) others++;
            }
            const bool red = obs > th_obs && others >= th_obs;
            nRed += red ? 1 : 0;
            if (entry_state) entry_state[(size_t)k * g.maxRow + i] = red ? 2 : 1;
        }
        counts[k].n_mps = nMPs, counts[k].n_redundant = nRed;
        redundant[k] = (double)nRed > 0.9 * (double)nMPs;
    }
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
