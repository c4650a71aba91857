// loopfuse_latency.cpp -- LoopClosing's two projection searches per call from a C++ caller, the path the library had before against
// the resident one (tools/loopfuse_latency.py runs it).  L key frames of N features on the far side of the
// loop hold older points of 6 N landmarks (their union is the loop list, about 4000 points at N = 1000, L = 8); K key frames on
// this side hold fresh points of the same landmarks and free features.  Every corrected pose is the key frame's own pose times a
// scale of 0.5, 1.37 or 2.  Per repetition, on the same map restored each time, alternating in one process:
//   SearchAndFuse over the K key frames
//     a  ORBmatcher::Fuse(pKF, Scw, ...) per key frame with the Replace loop behind it (the parent's path; ORBmatcher is unchanged)
//     b  LocalMapSearch::SearchAndFuse with points, rows and feature sets resident, the resident state kept up to date
//   SearchLoopPoints into the first of the K key frames
//     a  the union on the host, then ORBmatcher::SearchByProjection(pKF, Scw, ...)      b  LocalMapSearch::SearchLoopPoints
// a and b must leave the same map and the same matches, or the program fails.
// usage: loopfuse_latency N K L reps      prints "<name> median <us> p10 <us> p90 <us>" lines, "phase <name> <us per call>" lines of b,
// "floor <us>" (orbhip_debug_roundtrip mode 1 on the searching context) and "shape ..."
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "ORBmatcher.h"
#include "hiperror.h"
#include "orbhip.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 99;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 20) / (float)(1 << 20); }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static const int NLEVELS = 8, W = 752, H = 480;
static const float S = 1.2f, FX = 458.f, CX = 376.f, CY = 240.f;
static const float SCALES[3] = {0.5f, 1.37f, 2.0f};

static std::vector<KeyFrame *> g_kfs;                       // 0 .. K - 1: this side; K .. K + L - 1: the far side of the loop
static std::vector<MapPoint *> g_pts;
static std::vector<MapPoint> g_savedPts;                    // the map as built: restored before every timed call
static std::vector<std::vector<MapPoint *> > g_savedRows;

static MapPoint *new_point(const float P[3], const unsigned char *desc)
{
    MapPoint *p = new MapPoint();
    p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
    const float len = std::sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
    for (int k = 0; k < 3; k++) p->mWorldPos.at<float>(k, 0) = P[k], p->mNormalVector.at<float>(k, 0) = P[k] / len;
    memcpy(p->mDescriptor.ptr(0), desc, 32);
    p->mfMaxDistance = 12.f, p->mfMinDistance = 12.f / powf(S, NLEVELS - 1);
    g_pts.push_back(p);
    return p;
}

static void build(int N, int K, int L)
{
    const int NLM = 6 * N;
    std::vector<float> P((size_t)NLM * 3);
    std::vector<unsigned char> D((size_t)NLM * 32);
    for (int j = 0; j < NLM; j++) {
        const float z = frand(3, 12);
        P[3 * j] = (frand(20, W - 20) - CX) * z / FX, P[3 * j + 1] = (frand(20, H - 20) - CY) * z / FX, P[3 * j + 2] = z;
        for (int b = 0; b < 32; b++) D[(size_t)j * 32 + b] = (unsigned char)rnd(256);
    }
    std::vector<MapPoint *> oldOf(NLM, (MapPoint *)NULL), freshOf(NLM, (MapPoint *)NULL);
    for (int k = 0; k < K + L; k++) {
        KeyFrame *kf = new KeyFrame();
        g_kfs.push_back(kf);
        const bool far = k >= K;
        const float C[3] = {0.004f * k, 0.002f * (k % 5), 0.003f * (k % 7)};   // the neighbourhood of one place
        kf->Tcw = cv::Mat::zeros(4, 4, CV_32F), kf->Ow = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) kf->Tcw.at<float>(r, r) = 1.f, kf->Tcw.at<float>(r, 3) = -C[r], kf->Ow.at<float>(r, 0) = C[r];
        kf->Tcw.at<float>(3, 3) = 1.f;
        kf->fx = kf->fy = FX, kf->cx = CX, kf->cy = CY, kf->mbf = 0.f;
        kf->mnMinX = 0, kf->mnMaxX = W, kf->mnMinY = 0, kf->mnMaxY = H;
        kf->mfGridElementWidthInv = (float)FRAME_GRID_COLS / W, kf->mfGridElementHeightInv = (float)FRAME_GRID_ROWS / H;
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = S, kf->mfLogScaleFactor = logf(S);
        for (int l = 0; l < NLEVELS; l++) {
            kf->mvScaleFactors.push_back(powf(S, (float)l));
            kf->mvLevelSigma2.push_back(kf->mvScaleFactors[l] * kf->mvScaleFactors[l]);
            kf->mvInvLevelSigma2.push_back(1.0f / kf->mvLevelSigma2[l]);
        }
        kf->mDescriptors = cv::Mat(N, 32, CV_8U);
        kf->mvpMapPoints.assign(N, (MapPoint *)NULL);
        for (int i = 0; i < N; i++) {
            const int j = (int)rnd(NLM);            // (a landmark twice in a key frame: two features, as two detections would be)
            const float z = P[3 * j + 2] - C[2];
            const float u = FX * (P[3 * j] - C[0]) / z + CX + frand(-0.5f, 0.5f), v = FX * (P[3 * j + 1] - C[1]) / z + CY + frand(-0.5f, 0.5f);
            int oct = (int)floorf(logf(12.f / z) / logf(S));
            oct = oct < 0 ? 0 : oct > NLEVELS - 1 ? NLEVELS - 1 : oct;
            kf->mvKeys.push_back(cv::KeyPoint(u, v, 31.f * powf(S, (float)oct), frand(0, 360), 50.f, oct, -1));
            unsigned char *d = kf->mDescriptors.ptr(i);
            memcpy(d, &D[(size_t)j * 32], 32);
            for (int b = 0; b < 6; b++) d[rnd(32)] ^= (unsigned char)(1u << rnd(8));
            std::vector<MapPoint *> &of = far ? oldOf : freshOf;
            if (rnd(10) < 7) {                      // the landmark's point of this side of the loop, unless it is in this key frame already
                if (!of[j]) of[j] = new_point(&P[3 * j], d);
                if (!of[j]->IsInKeyFrame(kf)) kf->mvpMapPoints[i] = of[j], of[j]->AddObservation(kf, i);
            }
        }
        kf->mvKeysUn = kf->mvKeys;
        kf->N = N;
    }
    for (size_t i = 0; i < g_pts.size(); i++) g_savedPts.push_back(*g_pts[i]);
    for (size_t k = 0; k < g_kfs.size(); k++) g_savedRows.push_back(g_kfs[k]->mvpMapPoints);
}

static void restore(Probe *LS)
{
    for (size_t i = 0; i < g_pts.size(); i++) *g_pts[i] = g_savedPts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) g_kfs[k]->mvpMapPoints = g_savedRows[k];
    if (!LS) return;
    LS->Put(g_pts);
    for (size_t k = 0; k < g_kfs.size(); k++) LS->PutKeyFrame(g_kfs[k]);
}

static unsigned long long digest(const std::vector<MapPoint *> &extra)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < extra.size(); i++) h = (h ^ (extra[i] ? extra[i]->mnId + 1 : 0)) * 1099511628211ull;
    for (size_t k = 0; k < g_kfs.size(); k++)
        for (size_t i = 0; i < g_kfs[k]->mvpMapPoints.size(); i++)
            h = (h ^ (g_kfs[k]->mvpMapPoints[i] ? g_kfs[k]->mvpMapPoints[i]->mnId + 1 : 0)) * 1099511628211ull;
    for (size_t i = 0; i < g_pts.size(); i++) h = (h ^ ((unsigned long long)g_pts[i]->Observations() * 2 + (g_pts[i]->isBad() ? 1 : 0))) * 1099511628211ull;
    return h;
}

static cv::Mat similarity(KeyFrame *kf, float s)
{
    cv::Mat Scw = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) Scw.at<float>(r, c) = (float)((double)s * (double)kf->Tcw.at<float>(r, c));
    Scw.at<float>(3, 3) = 1.f;
    return Scw;
}

// ref: src/LoopClosing.cc:404-424 on the host (the stamp is a set)
static std::vector<MapPoint *> loop_points(const std::vector<KeyFrame *> &kfs)
{
    std::vector<MapPoint *> out;
    std::set<MapPoint *> stamped;
    for (size_t k = 0; k < kfs.size(); k++) {
        const std::vector<MapPoint *> vp = kfs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vp.size(); i++)
            if (vp[i] && !vp[i]->isBad() && stamped.insert(vp[i]).second) out.push_back(vp[i]);
    }
    return out;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 1000, K = argc > 2 ? atoi(argv[2]) : 10, L = argc > 3 ? atoi(argv[3]) : 8,
              reps = argc > 4 ? atoi(argv[4]) : 10;
    if (N < 16 || N > 8192 || K < 1 || L < 1 || K + L > 4000) return printf("usage: loopfuse_latency N K L reps\n"), 2;
    MapPoint::RecomputeOnReplace() = true;         // Replace ends in ComputeDistinctiveDescriptors, as in the reference
    build(N, K, L);
    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(K + L + 8, N);
    const std::vector<KeyFrame *> loopKFs(g_kfs.begin() + K, g_kfs.end());
    std::vector<std::pair<KeyFrame *, cv::Mat> > corrected;
    for (int k = 0; k < K; k++) corrected.push_back(std::make_pair(g_kfs[k], similarity(g_kfs[k], SCALES[k % 3])));
    const cv::Mat Scw0 = similarity(g_kfs[0], 1.37f);

    ORBmatcher matcher(0.8f);
    std::vector<double> t[4];
    unsigned long long want1 = 0, want2 = 0;
    long npoints = 0, nmatches = 0, replaced = 0;
    LocalMapSearch::Phases() = LocalMapSearch::LoopPhases();
    for (int r = -2; r < reps; r++) {
        if (r == 0) LocalMapSearch::Phases() = LocalMapSearch::LoopPhases();
        for (int mode = 0; mode < 2; mode++) {
            restore(mode == 1 ? &LS : NULL);
            std::vector<MapPoint *> list, matched(N, (MapPoint *)NULL);
            int nm = 0;
            Clock::time_point t0 = Clock::now();
            if (mode == 0) {
                list = loop_points(loopKFs);
                nm = matcher.SearchByProjection(g_kfs[0], Scw0, list, matched, 10);
            } else
                nm = LS.SearchLoopPoints(g_kfs[0], Scw0, loopKFs, list, matched, 10);
            double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            std::vector<MapPoint *> both(list);
            both.insert(both.end(), matched.begin(), matched.end());
            const unsigned long long d1 = digest(both);
            if (!want1) want1 = d1, npoints = (long)list.size(), nmatches = nm;
            if (d1 != want1) return printf("SearchLoopPoints, mode %d: another result\n", mode), 1;
            t0 = Clock::now();
            if (mode == 0) {
                for (size_t k = 0; k < corrected.size(); k++) {
                    std::vector<MapPoint *> vpReplacePoints(list.size(), static_cast<MapPoint *>(NULL));
                    matcher.Fuse(corrected[k].first, corrected[k].second, list, 4, vpReplacePoints);
                    for (size_t i = 0; i < list.size(); i++)
                        if (vpReplacePoints[i]) vpReplacePoints[i]->Replace(list[i]);
                }
            } else
                LS.SearchAndFuse(corrected, list, 4);
            us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[2 + mode].push_back(us);
            const unsigned long long d2 = digest(std::vector<MapPoint *>());
            if (!want2) {
                want2 = d2;
                for (size_t i = 0; i < g_pts.size(); i++) replaced += g_pts[i]->isBad() ? 1 : 0;
            }
            if (d2 != want2) return printf("SearchAndFuse, mode %d: another result\n", mode), 1;
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    const char *names[4] = {"looppoints_a_orbmatcher", "looppoints_b_resident", "fuse_a_orbmatcher", "fuse_b_resident"};
    for (int m = 0; m < 4; m++) report(names[m], t[m]);
    const LocalMapSearch::LoopPhases ph = LocalMapSearch::Phases();
    printf("phase prepare %.1f\nphase device %.1f\nphase research %.1f\nphase apply %.1f\nphase resident %.1f\n", ph.prepare / reps, ph.device / reps,
           ph.research / reps, ph.apply / reps, ph.resident / reps);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape features %d targets %d loop_kfs %d loop_points %ld matches %ld replaced %ld points %d\n", N, K, L, npoints, nmatches, replaced,
           (int)g_pts.size());
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
