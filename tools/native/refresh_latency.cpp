// refresh_latency.cpp -- what refreshing one key frame's map points costs a C++ caller (tools/refresh_latency.py; DESIGN.md section
// 19): N points, each seen from about OBS of K key frames, after a map edit that leaves every one of them to be recomputed.
//   a_host_put   MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth per point on the host, then LocalMapSearch::Put of
//                all of them: the path of the parent commit
//   b_refresh    LocalMapSearch::RefreshPoints: one orbhip_map_refresh call on the resident store and feature sets
//   c_host_only  the host loop alone, without the Put (what a map that is not resident pays)
// Before every timed call the objects and the store are put back to the same stale values (not timed).  The program fails unless a
// and b leave the same descriptors, normals and ranges in the objects.  Prints "<mode> median <us> p10 <us> p90 <us>" per mode,
// "floor <us>" (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 16) / 65536.f; }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;
static std::vector<MapPoint> g_saved;

static void build(int N, int K, int OBS)
{
    g_seed = 2024;
    const int NF = N + 200, NLEVELS = 8;
    std::vector<int> nextFree(K, 0);
    for (int k = 0; k < K; k++) {
        KeyFrame *kf = new KeyFrame();
        g_kfs.push_back(kf);
        kf->N = NF;
        kf->Ow = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) kf->Ow.at<float>(c, 0) = frand(-3.f, 3.f);
        kf->Tcw = cv::Mat::zeros(4, 4, CV_32F);
        kf->mnMinX = 0, kf->mnMaxX = 640, kf->mnMinY = 0, kf->mnMaxY = 480;
        kf->mfGridElementWidthInv = 64.f / 640.f, kf->mfGridElementHeightInv = 48.f / 480.f;
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = 1.2f, kf->mfLogScaleFactor = logf(1.2f);
        float s = 1.f;
        for (int l = 0; l < NLEVELS; l++, s *= 1.2f) {
            kf->mvScaleFactors.push_back(s);
            kf->mvLevelSigma2.push_back(s * s);
            kf->mvInvLevelSigma2.push_back(1.f / (s * s));
        }
        kf->mDescriptors = cv::Mat(NF, 32, CV_8U);
        for (int i = 0; i < NF; i++) {
            kf->mvKeys.push_back(cv::KeyPoint(frand(2, 637), frand(2, 477), 31.f, frand(0, 360), 20.f, (int)rnd(NLEVELS), -1));
            for (int b = 0; b < 32; b++) kf->mDescriptors.ptr(i)[b] = (uint8_t)rnd(256);
        }
        kf->mvKeysUn = kf->mvKeys;
        kf->mvpMapPoints.assign(NF, (MapPoint *)NULL);
    }
    for (int j = 0; j < N; j++) {
        MapPoint *p = new MapPoint();
        g_pts.push_back(p);
        p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c, 0) = frand(-6.f, 6.f) + (c == 2 ? 9.f : 0.f), p->mNormalVector.at<float>(c, 0) = 0.f;
        uint8_t base[32];
        for (int b = 0; b < 32; b++) base[b] = p->mDescriptor.ptr(0)[b] = (uint8_t)rnd(256);
        p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
        const int n = std::max(1, std::min(K, OBS - 2 + (int)rnd(5)));      // OBS on average
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 200; tries++) {
            const int k = p->mObservations.empty() ? 0 : (int)rnd(K);       // the key frame being refreshed sees every point
            KeyFrame *kf = g_kfs[k];
            if (p->IsInKeyFrame(kf) || nextFree[k] >= kf->N) continue;
            const int idx = nextFree[k]++;
            uint8_t *d = kf->mDescriptors.ptr(idx);
            memcpy(d, base, 32);
            for (unsigned b = rnd(6); b > 0; b--) d[rnd(32)] ^= (uint8_t)(1u << rnd(8));
            kf->mvpMapPoints[idx] = p;
            p->AddObservation(kf, idx);
            if (!p->mpRefKF) p->mpRefKF = kf;
        }
    }
    for (size_t i = 0; i < g_pts.size(); i++) g_saved.push_back(*g_pts[i]);
}

static unsigned long long digest()
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < g_pts.size(); i++) {
        MapPoint *p = g_pts[i];
        unsigned u[5];
        for (int c = 0; c < 3; c++) memcpy(&u[c], &p->mNormalVector.at<float>(c, 0), 4);
        memcpy(&u[3], &p->mfMinDistance, 4), memcpy(&u[4], &p->mfMaxDistance, 4);
        for (int c = 0; c < 5; c++) h = (h ^ u[c]) * 1099511628211ull;
        for (int b = 0; b < 32; b++) h = (h ^ p->mDescriptor.ptr(0)[b]) * 1099511628211ull;
    }
    return h;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 1000, K = argc > 2 ? atoi(argv[2]) : 20, OBS = argc > 3 ? atoi(argv[3]) : 6,
              reps = argc > 4 ? atoi(argv[4]) : 30;
    if (N < 1 || N > 100000 || K < 1 || K > 90 || OBS < 1 || reps < 1) return printf("usage: refresh_latency N K OBS reps (K <= 90)\n"), 2;
    build(N, K, OBS);
    Probe LS(N + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    std::vector<double> t[3];
    unsigned long long want = 0;
    long nobs = 0;
    for (size_t i = 0; i < g_pts.size(); i++) nobs += (long)g_pts[i]->mObservations.size();
    for (int r = -3; r < reps; r++) {
        for (int mode = 0; mode < 3; mode++) {
            for (size_t i = 0; i < g_pts.size(); i++) *g_pts[i] = g_saved[i];     // the stale values, in the objects and in the store
            LS.Put(g_pts);
            const Clock::time_point t0 = Clock::now();
            if (mode == 1)
                LS.RefreshPoints(g_pts);
            else {
                for (size_t i = 0; i < g_pts.size(); i++) {
                    g_pts[i]->ComputeDistinctiveDescriptors();
                    g_pts[i]->UpdateNormalAndDepth();
                }
                if (mode == 0) LS.Put(g_pts);
            }
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            const unsigned long long d = digest();
            if (!want) want = d;
            if (d != want) return printf("mode %d: another result\n", mode), 1;
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    if (LocalMapSearch::RefreshCounts().host != 0) return printf("points went the host way: the measurement is not of the device call\n"), 1;
    const char *names[3] = {"a_host_put", "b_refresh", "c_host_only"};
    for (int m = 0; m < 3; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape points %d key_frames %d observations %ld\n", N, K, nobs);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
