// baproblem_latency.cpp -- what the set-up of Optimizer::LocalBundleAdjustment costs a C++ caller (tools/baproblem_latency.py;
// DESIGN.md section 24): a map of NKF key frames of NFEAT features, every point seen from about six key frames of a neighbourhood;
// the key frame in the middle of the map runs local bundle adjustment with its K - 1 nearest key frames as covisibility list.
//   a_host    the reference's three loops on slamlite.h objects (tests/native_baproblem/ref_ba.h): the local key frames, the
//             points, the fixed key frames, and (pKF, idx) pushed where the reference allocates an edge -- the baseline
//   b_dropin  LocalMapSearch::BuildLocalBA: the list, one device call, keys and indices turned into pointers, the stamps
//   c_call    orbhip_map_ba_problem alone, with exact room
// The stamps of both are put back before every call, not timed (the reference's walk takes no point that carries this run's
// stamp).  The program fails unless a and b give the same five vectors.  Prints "<mode> median <us> p10 <us> p90 <us>" per mode,
// "floor <us>" (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_ba.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;

static void build(int NKF, int NFEAT, int OBS, int WINDOW)
{
    g_seed = 2025;
    std::vector<int> nextFree(NKF, 0);
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        kf->mnId = (long unsigned int)k;
        kf->N = NFEAT;
        kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
        kf->mvKeysUn.resize(NFEAT);
        kf->mvuRight.assign(NFEAT, -1.f);
        kf->mvDepth.assign(NFEAT, -1.f);
        g_kfs.push_back(kf);
    }
    const int NPT = (int)((long)NKF * NFEAT / OBS);
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new MapPoint();
        p->mnId = (long unsigned int)j;
        p->mWorldPos = cv::Mat::zeros(3, 1, CV_32F), p->mNormalVector = cv::Mat::zeros(3, 1, CV_32F), p->mDescriptor = cv::Mat::zeros(1, 32, CV_8U);
        g_pts.push_back(p);
        const int n = std::max(1, OBS - 2 + (int)rnd(5)), centre = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 100; tries++) {
            const int k = centre - WINDOW + (int)rnd(2 * WINDOW + 1);
            if (k < 0 || k >= NKF || p->IsInKeyFrame(g_kfs[k]) || nextFree[k] >= NFEAT) continue;
            const int idx = nextFree[k]++;
            g_kfs[k]->mvpMapPoints[idx] = p;
            p->AddObservation(g_kfs[k], idx);
        }
    }
}

static void reset_stamps()
{
    for (size_t k = 0; k < g_kfs.size(); k++) g_kfs[k]->mnBALocalForKF = g_kfs[k]->mnBAFixedForKF = ~0ul;
    for (size_t j = 0; j < g_pts.size(); j++) g_pts[j]->mnBALocalForKF = ~0ul;
}

static bool same(const LocalMapSearch::BAProblem &a, const refba::Problem &b)
{
    if (a.vpLocalKFs != b.vpLocalKFs || a.vpFixedKFs != b.vpFixedKFs || a.vpLocalMPs != b.vpLocalMPs || a.vEdgeOff != b.vEdgeOff ||
        a.vEdges.size() != b.vEdges.size())
        return false;
    for (size_t i = 0; i < a.vEdges.size(); i++)
        if (a.vEdges[i].pKF != b.vEdges[i].pKF || a.vEdges[i].idx != b.vEdges[i].idx) return false;
    return true;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int K = argc > 1 ? atoi(argv[1]) : 20, reps = argc > 2 ? atoi(argv[2]) : 30, NKF = argc > 3 ? atoi(argv[3]) : 200,
              NFEAT = argc > 4 ? atoi(argv[4]) : 1000;
    if (K < 2 || K > NKF || reps < 1 || NKF < 8 || NKF > 4096 || NFEAT < 1 || NFEAT > 8192)
        return printf("usage: baproblem_latency K reps [key frames <= 4096] [features <= 8192]\n"), 2;
    build(NKF, NFEAT, 6, 10);
    KeyFrame *pKF = g_kfs[NKF / 2];
    for (int d = 1; (int)pKF->mvpOrderedConnectedKeyFrames.size() < K - 1; d++) {   // nearest first, as by weight
        if (NKF / 2 + d < NKF) pKF->mvpOrderedConnectedKeyFrames.push_back(g_kfs[NKF / 2 + d]);
        if ((int)pKF->mvpOrderedConnectedKeyFrames.size() < K - 1 && NKF / 2 - d >= 0) pKF->mvpOrderedConnectedKeyFrames.push_back(g_kfs[NKF / 2 - d]);
    }

    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(NKF, NFEAT);
    LS.Put(g_pts);
    for (int k = 0; k < NKF; k++) LS.PutKeyFrame(g_kfs[k]);

    LocalMapSearch::BAProblem out;
    refba::Problem ref;
    reset_stamps();
    refba::Build(refba::LocalKeyFrames(pKF), pKF->mnId, ref);
    reset_stamps();
    if (!LS.BuildLocalBA(pKF, out)) return printf("BuildLocalBA failed: %s\n", OrbHipLastError()), 1;
    if (!same(out, ref)) return printf("BuildLocalBA and the reference's loops differ\n"), 1;
    std::vector<uint64_t> keys, ptKeys(out.vpLocalMPs.size() + 1), fixedKeys(out.vpFixedKFs.size() + 1);
    for (size_t i = 0; i < out.vpLocalKFs.size(); i++) keys.push_back((uint64_t)out.vpLocalKFs[i]->mnId + 1);
    std::vector<int32_t> off(out.vpLocalMPs.size() + 1);
    std::vector<orbhip_ba_edge> edges(out.vEdges.size() + 1);
    const int capP = (int)out.vpLocalMPs.size(), capE = (int)out.vEdges.size(), capF = (int)out.vpFixedKFs.size();

    std::vector<double> t[3];
    for (int r = -3; r < reps; r++) {
        for (int mode = 0; mode < 3; mode++) {
            reset_stamps();
            int np = 0, ne = 0, nf = 0;
            const Clock::time_point t0 = Clock::now();
            if (mode == 0)
                refba::Build(refba::LocalKeyFrames(pKF), pKF->mnId, ref);
            else if (mode == 1) {
                if (!LS.BuildLocalBA(pKF, out)) return printf("BuildLocalBA failed: %s\n", OrbHipLastError()), 1;
            } else if (orbhip_map_ba_problem(LS.ctx(), (int)keys.size(), keys.data(), ptKeys.data(), capP, &np, off.data(), edges.data(), capE, &ne,
                                             fixedKeys.data(), capF, &nf) != ORBHIP_OK)
                return printf("orbhip_map_ba_problem failed: %s\n", orbhip_last_error(LS.ctx())), 1;
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            if (mode == 2 && (np != capP || ne != capE || nf != capF)) return printf("the call's counts changed\n"), 1;
        }
    }
    if (!same(out, ref)) return printf("BuildLocalBA and the reference's loops differ\n"), 1;
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    const char *names[3] = {"a_host", "b_dropin", "c_call"};
    for (int m = 0; m < 3; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape key_frames %d features %d points %d local %d local_points %d edges %d fixed %d\n", NKF, NFEAT, (int)g_pts.size(), K, capP, capE,
           capF);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
