// mock_bowcand.cc -- a host model of the entry points ORB_SLAM2::LocalMapSearch::SearchByBoWCandidates calls, for the programs that
// run it without a device (test_bowcand_mock, test_bowcand_mock_asan).  The store keeps position, flags and an incarnation number per
// point key; a key-frame row keeps (point key, incarnation) per entry, so that an entry whose point was erased, cleared away or
// put again resolves to nothing -- what the slot and its generation do in the library; a set keeps keypoints, descriptors and the
// FeatureVector.  orbhip_search_by_bow_candidates walks the shared nodes as the header says, with the library's argument checks.
// ORBmatcher::SearchByBoW, the host way of the class, is the reference loop of ref_bowcand.h here (the library's own lives in
// liborbhip_host.so and needs a device).  The entry points the class links but these programs never reach fail loudly.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "ORBmatcher.h"
#include "orbhip.h"
#include "ref_bowcand.h"
#include "slamlite.h"

namespace
{
struct Point {
    uint8_t flags;
    unsigned long born;
    float pos[3];
};
typedef std::pair<uint64_t, unsigned long> Entry;   // point key (0: none), incarnation
struct Set {
    std::vector<orbhip_keypoint> kps;
    std::vector<uint8_t> desc;
    std::vector<int32_t> node, off, idx;
    unsigned long stamp;
};
struct Mock {
    int maxPoints = 0, maxKfs = 0, maxRow = 0, setLimit = 96;
    bool table = false;
    unsigned long clock = 0;
    std::map<uint64_t, Point> points;
    std::map<uint64_t, std::vector<Entry> > rows;
    std::map<uint64_t, Set> sets;
} g;

const Point *resolve(const Entry &e)
{
    if (!e.first) return NULL;
    std::map<uint64_t, Point>::const_iterator it = g.points.find(e.first);
    return it != g.points.end() && it->second.born == e.second && !(it->second.flags & ORBHIP_MP_BAD) ? &it->second : NULL;
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
    fprintf(stderr, "mock_bowcand: %s is not modelled\n", who);
    return ORBHIP_E_ARG;
}

int dist(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

// one pair: side 1 / side 2 sets with a validity test each; m12 [n1], m21 [n2] come back, the return value is the match count
struct Side {
    const Set *s;
    const std::vector<Entry> *row;   // NULL: every feature counts
    bool valid(int i) const { return !row || resolve((*row)[i]) != NULL; }
};
int pair_search(const Side &A, const Side &B, int th, int strict, float nnratio, int check_ori, std::vector<int32_t> &m12, std::vector<int32_t> &m21)
{
    m12.assign(A.s->kps.size(), -1), m21.assign(B.s->kps.size(), -1);
    std::vector<int> hist[30];
    int nm = 0;
    for (size_t g1 = 0, g2 = 0; g1 < A.s->node.size() && g2 < B.s->node.size();) {
        if (A.s->node[g1] < B.s->node[g2]) { g1++; continue; }
        if (A.s->node[g1] > B.s->node[g2]) { g2++; continue; }
        for (int a = A.s->off[g1]; a < A.s->off[g1 + 1]; a++) {
            const int i1 = A.s->idx[a];
            if (!A.valid(i1)) continue;
            int b1 = 256, b2 = 256, bi = -1;
            for (int b = B.s->off[g2]; b < B.s->off[g2 + 1]; b++) {
                const int i2 = B.s->idx[b];
                if (m21[i2] >= 0 || !B.valid(i2)) continue;
                const int d = dist(&A.s->desc[(size_t)i1 * 32], &B.s->desc[(size_t)i2 * 32]);
                if (d < b1) b2 = b1, b1 = d, bi = i2;
                else if (d < b2) b2 = d;
            }
            if ((strict ? b1 < th : b1 <= th) && (float)b1 < nnratio * (float)b2) {
                m12[i1] = bi, m21[bi] = i1, nm++;
                if (check_ori) {
                    float rot = A.s->kps[i1].angle - B.s->kps[bi].angle;
                    if (rot < 0.0f) rot += 360.0f;
                    int bin = (int)roundf(rot * (1.0f / 30));
                    if (bin == 30) bin = 0;
                    if (bin >= 0 && bin < 30) hist[bin].push_back(i1);
                }
            }
        }
        g1++, g2++;
    }
    if (check_ori) {
        int k1, k2, k3;
        refbow::three_maxima(hist, 30, k1, k2, k3);
        for (int i = 0; i < 30; i++) {
            if (i == k1 || i == k2 || i == k3) continue;
            for (size_t j = 0; j < hist[i].size(); j++) m21[m12[hist[i][j]]] = -1, m12[hist[i][j]] = -1, nm--;
        }
    }
    return nm;
}
}  // namespace

extern "C" {
orbhip_ctx *orbhip_create(int, int, float, int, int, int, int, int, int) { return (orbhip_ctx *)&g; }
void orbhip_destroy(orbhip_ctx *) {}
const char *orbhip_last_error(const orbhip_ctx *) { return "mock error"; }
int orbhip_map_init(orbhip_ctx *, int max_points) { g = Mock(); g.maxPoints = max_points; return ORBHIP_OK; }
int orbhip_map_clear(orbhip_ctx *) { g.points.clear(); return ORBHIP_OK; }
int orbhip_map_put(orbhip_ctx *, int n, const uint64_t *keys, const float *pos, const float *, const float *, const float *, const uint8_t *,
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
        Point &p = g.points[keys[i]];
        p.flags = flags[i];
        memcpy(p.pos, pos + 3 * (size_t)i, 12);
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

// ---- resident sets: least recently used out, as the library's table ----
int orbhip_set_limit(orbhip_ctx *, int n)
{
    g.setLimit = n < 4 ? 4 : n > 96 ? 96 : n;
    return g.setLimit;
}
int orbhip_set_drop(orbhip_ctx *, uint64_t key)
{
    if (key) g.sets.erase(key);
    else g.sets.clear();
    return ORBHIP_OK;
}
int orbhip_set_has(orbhip_ctx *, uint64_t key, int n) { return g.sets.count(key) && (int)g.sets[key].kps.size() == n ? 1 : 0; }
uint64_t orbhip_set_fingerprint_rows(const orbhip_keypoint *first_kp, const uint8_t *first_desc, const uint8_t *last_desc, int n)
{
    uint64_t h = 1469598103934665603ull ^ (uint64_t)n;
    const uint8_t *parts[3] = {reinterpret_cast<const uint8_t *>(first_kp), first_desc, last_desc};
    const size_t len[3] = {8, 32, 32};
    for (int p = 0; p < 3; p++)
        for (size_t k = 0; k < len[p]; k++) h = (h ^ parts[p][k]) * 1099511628211ull;
    return h;
}
int orbhip_set_info(orbhip_ctx *, uint64_t key, int *n, int *ng, uint64_t *fingerprint)
{
    std::map<uint64_t, Set>::iterator it = g.sets.find(key);
    if (it == g.sets.end()) return 0;
    Set &s = it->second;
    s.stamp = ++g.clock;
    const int cnt = (int)s.kps.size();
    if (n) *n = cnt;
    if (ng) *ng = (int)s.node.size();
    if (fingerprint) *fingerprint = orbhip_set_fingerprint_rows(&s.kps[0], &s.desc[0], &s.desc[(size_t)(cnt - 1) * 32], cnt);
    return 1;
}
int orbhip_set_put(orbhip_ctx *, uint64_t key, const orbhip_keypoint *kps, const uint8_t *desc, int n, const int32_t *node, const int32_t *off,
                   const int32_t *idx, int ng, float, float, float, float)
{
    if (!key || n <= 0 || !kps || !desc || ng < 0 || ng > n) return ORBHIP_E_ARG;
    Set s;
    s.kps.assign(kps, kps + n), s.desc.assign(desc, desc + (size_t)n * 32);
    if (ng > 0) s.node.assign(node, node + ng), s.off.assign(off, off + ng + 1), s.idx.assign(idx, idx + off[ng]);
    else s.off.assign(1, 0);
    s.stamp = ++g.clock;
    g.sets.erase(key);
    while ((int)g.sets.size() >= g.setLimit) {
        std::map<uint64_t, Set>::iterator old = g.sets.begin();
        for (std::map<uint64_t, Set>::iterator it = g.sets.begin(); it != g.sets.end(); ++it)
            if (it->second.stamp < old->second.stamp) old = it;
        g.sets.erase(old);
    }
    g.sets[key] = s;
    return ORBHIP_OK;
}
uint64_t orbhip_frame_fingerprint(const orbhip_ctx *) { return 0; }
int orbhip_set_put_from_frame(orbhip_ctx *, uint64_t, orbhip_ctx *, const int32_t *, const int32_t *, const int32_t *, int)
{
    return unreachable("orbhip_set_put_from_frame");
}

int orbhip_search_by_bow_candidates(orbhip_ctx *, int mode, uint64_t fixed_set_key, uint64_t fixed_row_key, const orbhip_bow_candidate *cand, int K,
                                    int th, float nnratio, int check_ori, int32_t *matches, int32_t *nmatches, int min_matches,
                                    const float *level_sigma2, int nlevels, float th2, int32_t *off, int32_t *kp_idx, int32_t *kf_idx, float *P3Dw,
                                    float *P2D, float *max_err, int cap, int *ntotal)
{
    if (K < 0 || (mode != 0 && mode != 1)) return ORBHIP_E_ARG;
    if (K == 0) return ORBHIP_OK;
    if (!cand || !matches || !nmatches || K > 4095 || !g.table) return ORBHIP_E_ARG;
    const bool any = level_sigma2 || off || kp_idx || kf_idx || P3Dw || P2D || max_err || ntotal;
    const bool gather = level_sigma2 && off && kp_idx && kf_idx && P3Dw && P2D && max_err && ntotal;
    if (any && (!gather || mode != 0 || cap < 0 || nlevels < 1 || nlevels > 64)) return ORBHIP_E_ARG;
    std::set<uint64_t> distinct;
    distinct.insert(fixed_set_key);
    for (int k = 0; k < K; k++) distinct.insert(cand[k].set_key);
    if ((int)distinct.size() > g.setLimit) return ORBHIP_E_ARG;
    if (!g.sets.count(fixed_set_key)) return ORBHIP_E_ARG;
    const Set &F = g.sets[fixed_set_key];
    const int nF = (int)F.kps.size();
    const std::vector<Entry> *rowF = NULL;
    if (mode == 1) {
        if (!g.rows.count(fixed_row_key) || (int)g.rows[fixed_row_key].size() != nF) return ORBHIP_E_ARG;
        rowF = &g.rows[fixed_row_key];
    }
    for (int k = 0; k < K; k++) {
        if (!g.sets.count(cand[k].set_key) || !g.rows.count(cand[k].row_key)) return ORBHIP_E_ARG;
        if (g.rows[cand[k].row_key].size() != g.sets[cand[k].set_key].kps.size()) return ORBHIP_E_ARG;
    }
    if (gather)
        for (int i = 0; i < nF; i++)
            if (F.kps[i].octave < 0 || F.kps[i].octave >= nlevels) return ORBHIP_E_ARG;
    std::vector<std::vector<int32_t> > rows(K);
    std::vector<int> nm(K);
    std::vector<int32_t> other;
    int total = 0;
    for (int k = 0; k < K; k++) {
        const Side C = {&g.sets[cand[k].set_key], &g.rows[cand[k].row_key]}, Fx = {&F, rowF};
        nm[k] = mode == 0 ? pair_search(C, Fx, th, 0, nnratio, check_ori, other, rows[k]) : pair_search(Fx, C, th, 1, nnratio, check_ori, rows[k], other);
        if (gather && nm[k] >= min_matches) total += nm[k];
    }
    if (gather) {
        *ntotal = total;
        if (total > cap) return ORBHIP_E_CAPACITY;
        int at = 0;
        for (int k = 0; k < K; k++) {
            off[k] = at;
            if (nm[k] < min_matches) continue;
            const std::vector<Entry> &row = g.rows[cand[k].row_key];
            for (int i = 0; i < nF; i++) {
                const int j = rows[k][i];
                if (j < 0) continue;
                const Point *p = resolve(row[j]);
                kp_idx[at] = i, kf_idx[at] = j;
                P2D[2 * at] = F.kps[i].x, P2D[2 * at + 1] = F.kps[i].y;
                max_err[at] = level_sigma2[F.kps[i].octave] * th2;
                for (int c = 0; c < 3; c++) P3Dw[3 * at + c] = p ? p->pos[c] : 0.f;
                at++;
            }
        }
        off[K] = at;
    }
    for (int k = 0; k < K; k++) {
        memcpy(matches + (size_t)k * nF, rows[k].data(), (size_t)nF * 4);
        nmatches[k] = nm[k];
    }
    return ORBHIP_OK;
}

// linked by LocalMap.cc, LocalMapCollect.cc and LocalMapFuse.cc, never reached by these programs
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
int orbhip_fuse_row(orbhip_ctx *, uint64_t, const orbhip_fuse_target *, int, const uint8_t *, const float *, orbhip_proj_query *, int32_t *,
                    int32_t *, int32_t *)
{
    return unreachable("orbhip_fuse_row");
}
int orbhip_fuse_collect(orbhip_ctx *, const orbhip_fuse_target *, uint64_t, int, const uint64_t *, const float *, uint64_t *, int, int *,
                        orbhip_proj_query *, int32_t *, int32_t *, int *)
{
    return unreachable("orbhip_fuse_collect");
}
int orbhip_window_best_set(orbhip_ctx *, uint64_t, const float *, const float *, int, const orbhip_proj_query *, const uint8_t *, int, int32_t *,
                           int32_t *)
{
    return unreachable("orbhip_window_best_set");
}
}

namespace ORB_SLAM2
{
// the Frame statics that host/FrameGrid.cc defines in liborbhip_host.so (these programs link neither)
float Frame::fx, Frame::fy, Frame::cx, Frame::cy;
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
float Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;

// the host way of the class in these programs
const int ORBmatcher::TH_LOW = 50;
const int ORBmatcher::TH_HIGH = 100;
const int ORBmatcher::HISTO_LENGTH = 30;
ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
ORBmatcher::~ORBmatcher() {}
int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint *> &vpMapPointMatches)
{
    return refbow::SearchByBoW(pKF, F, vpMapPointMatches, mfNNratio, mbCheckOrientation);
}
int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12)
{
    return refbow::SearchByBoW(pKF1, pKF2, vpMatches12, mfNNratio, mbCheckOrientation);
}
}  // namespace ORB_SLAM2
