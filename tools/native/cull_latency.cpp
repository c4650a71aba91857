// cull_latency.cpp -- what LocalMapping::KeyFrameCulling over K covisible key frames costs a C++ caller (tools/cull_latency.py;
// DESIGN.md section 22): a map of NKF key frames of NFEAT features, every point seen from about six key frames of a neighbourhood at
// octaves 0..7, the K key frames in the middle of the map as vpLocalKeyFrames.  Two of them hold every feature at octave 7, so that
// every observer of their points is "at the same or a finer scale": they are the two that are culled; nothing else is redundant.
//   a0_host    the reference loop on slamlite.h objects (tests/native_cull/ref_cull.h), the two skipped: 0 culls -- the baseline of b
//   a2_host    the same with nothing skipped: 2 culls -- the baseline of c
//   b_dropin0  LocalMapSearch::KeyFrameCulling, the two skipped: one device call, 0 culls
//   c_dropin2  the same with nothing skipped: 2 culls, three device calls
//   d_call     orbhip_map_cull alone for the K key frames
// After every call that culled, the objects are restored from a snapshot and the resident state is brought back (rows, flags,
// levels), not timed.  The program fails unless a and the drop-in cull the same key frames.  Prints "<mode> median <us> p10 <us>
// p90 <us>" per mode, "floor <us>" (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_cull.h"

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

static void build(int NKF, int NFEAT, int OBS, int WINDOW, int coarse0, int coarse1)
{
    g_seed = 2025;
    std::vector<int> nextFree(NKF, 0);
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        kf->mnId = (long unsigned int)k;
        kf->N = NFEAT;
        kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
        kf->mvKeysUn.resize(NFEAT);
        for (int i = 0; i < NFEAT; i++) kf->mvKeysUn[i].octave = (k == coarse0 || k == coarse1) ? 7 : (int)rnd(8);
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

struct SkipTwo {
    KeyFrame *a, *b;
    bool on;
    bool operator()(KeyFrame *pKF) const { return on && (pKF == a || pKF == b); }
};
struct SetBad {
    std::vector<KeyFrame *> *culled;
    void operator()(KeyFrame *pKF) const
    {
        pKF->SetBadFlag();
        culled->push_back(pKF);
    }
};

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
    if (K < 4 || K > NKF || reps < 1 || NKF < 8 || NKF > 4096 || NFEAT < 1 || NFEAT > 8192)
        return printf("usage: cull_latency K reps [key frames <= 4096] [features <= 8192]\n"), 2;
    const int first = (NKF - K) / 2, c0 = first + K / 3, c1 = first + (2 * K) / 3;
    build(NKF, NFEAT, 6, 10, c0, c1);
    // the snapshot the objects are restored from after a call that culled
    std::vector<MapPoint> snapPts;
    std::vector<std::vector<MapPoint *> > snapRows;
    for (size_t i = 0; i < g_pts.size(); i++) snapPts.push_back(*g_pts[i]);
    for (size_t k = 0; k < g_kfs.size(); k++) snapRows.push_back(g_kfs[k]->mvpMapPoints);

    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(NKF, NFEAT);
    LS.Put(g_pts);
    for (int k = 0; k < NKF; k++) LS.PutKeyFrame(g_kfs[k]);
    std::vector<KeyFrame *> batch;
    std::vector<uint64_t> keys;
    for (int i = 0; i < K; i++) {
        batch.push_back(g_kfs[first + i]);
        keys.push_back((uint64_t)g_kfs[first + i]->mnId + 1);
    }
    std::vector<LocalMapSearch::CullCount> warm;
    if (!LS.CullCounts(batch, true, warm)) return printf("CullCounts failed: %s\n", OrbHipLastError()), 1;   // (the levels travel here)
    std::vector<orbhip_cull_count> counts(K);
    std::vector<uint8_t> red(K);
    std::vector<double> t[5];
    long entries = 0;
    for (int i = 0; i < K; i++) entries += warm[i].nMPs;
    for (int r = -3; r < reps; r++) {
        for (int mode = 0; mode < 5; mode++) {
            std::vector<KeyFrame *> culled;
            const SkipTwo skip = {g_kfs[c0], g_kfs[c1], mode == 0 || mode == 2};
            const SetBad cull = {&culled};
            const Clock::time_point t0 = Clock::now();
            if (mode == 0 || mode == 1)
                culled = refcull::KeyFrameCulling(batch, true, skip);
            else if (mode == 2 || mode == 3)
                LS.KeyFrameCulling(batch, true, skip, cull);
            else if (orbhip_map_cull(LS.ctx(), K, keys.data(), 1, 3, counts.data(), red.data(), NULL) != ORBHIP_OK)
                return printf("orbhip_map_cull failed: %s\n", orbhip_last_error(LS.ctx())), 1;
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            const bool two = mode == 1 || mode == 3;
            if (mode != 4 && (culled.size() != (two ? 2u : 0u) || (two && (culled[0] != g_kfs[c0] || culled[1] != g_kfs[c1]))))
                return printf("mode %d: %d key frames culled\n", mode, (int)culled.size()), 1;
            if (!two) continue;
            // ---- not timed: the map as it was ----
            std::vector<MapPoint *> turned;
            for (size_t i = 0; i < g_pts.size(); i++) {
                if (g_pts[i]->isBad()) turned.push_back(g_pts[i]);
                if (g_pts[i]->Observations() != snapPts[i].Observations() || g_pts[i]->isBad()) *g_pts[i] = snapPts[i];
            }
            for (size_t k = 0; k < g_kfs.size(); k++) g_kfs[k]->mvpMapPoints = snapRows[k], g_kfs[k]->mbBad = false;
            if (mode == 3) {
                for (size_t i = 0; i < turned.size(); i++) LS.UpdateFlags(turned[i]);
                LS.PutKeyFrame(g_kfs[c0]), LS.PutKeyFrame(g_kfs[c1]);
                if (!LS.CullCounts(batch, true, warm)) return printf("CullCounts failed: %s\n", OrbHipLastError()), 1;
            }
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    if (LocalMapSearch::CullWayCounts().host != 0) return printf("key frames went the host way: the measurement is not of the device call\n"), 1;
    const char *names[5] = {"a0_host", "a2_host", "b_dropin0", "c_dropin2", "d_call"};
    for (int m = 0; m < 5; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    long nobs = 0;
    for (size_t i = 0; i < g_pts.size(); i++) nobs += (long)g_pts[i]->mObservations.size();
    printf("shape key_frames %d features %d points %d observations %ld candidates %d counted %ld\n", NKF, NFEAT, (int)g_pts.size(), nobs, K, entries);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
