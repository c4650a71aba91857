// projtrack_latency.cpp -- Tracking's two other projection searches per call from a C++ caller, the path the library had
// before against the resident one (tools/projtrack_latency.py runs it).  N source features with a map
// point each (9 in 10) against a 752 x 480 frame of N features.  Per repetition, alternating in one process, for the last-frame
// form (SearchByProjection(CurrentFrame, LastFrame, th, bMono)) and the key-frame form (SearchByProjection(CurrentFrame, pKF,
// sAlreadyFound, th, ORBdist)):
//   a  ORBmatcher's method as it stands: every point read and projected on the host, queries, descriptors and the whole
//      current frame uploaded (the parent's path; ORBmatcher is unchanged)
//   b  LocalMapSearch::SearchLastFrame / SearchKeyFramePoints with both frames, the points and the row resident
//   c  the same with the frames' sets dropped before the call (put cold inside it)
//   d  the restated host loop with the oracle's window search on one core (tests/native_projtrack/ref_projtrack.h)
// a, b and d must leave the same matches and counts, or the program fails.
// usage: projtrack_latency N reps      prints "<name> median <us> p10 <us> p90 <us>" lines, "floor <us>" (orbhip_debug_roundtrip
// mode 1 on the searching context) and "shape ..."
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
#include "ref_projtrack.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 77;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 20) / (float)(1 << 20); }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static const int NLEVELS = 8, W = 752, H = 480;
static const float S = 1.2f;

static void frame_common(Frame &F)
{
    F.mTcw = cv::Mat::zeros(4, 4, CV_32F);
    for (int k = 0; k < 4; k++) F.mTcw.at<float>(k, k) = 1.f;
    F.mnScaleLevels = NLEVELS, F.mfScaleFactor = S, F.mfLogScaleFactor = logf(S);
    for (int l = 0; l < NLEVELS; l++) F.mvScaleFactors.push_back(powf(S, (float)l));
    F.mbf = 40.f, F.mb = 0.08f;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 1000, reps = argc > 2 ? atoi(argv[2]) : 100;
    Frame::fx = 458, Frame::fy = 457, Frame::cx = 376, Frame::cy = 240;
    Frame::mnMinX = 0, Frame::mnMaxX = W, Frame::mnMinY = 0, Frame::mnMaxY = H;
    Frame::mfGridElementWidthInv = (float)FRAME_GRID_COLS / W, Frame::mfGridElementHeightInv = (float)FRAME_GRID_ROWS / H;
    Probe LS(4 * N + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(4, N);

    Frame Cur, Last;
    frame_common(Cur), frame_common(Last);
    Cur.mTcw.at<float>(2, 3) = -0.12f;      // the camera moved forward by more than the baseline
    std::vector<MapPoint *> pts;
    cv::Mat dc(N, 32, CV_8U), dl(N, 32, CV_8U);
    for (int i = 0; i < N; i++) {
        const float u = frand(4, W - 4), v = frand(4, H - 4), z = frand(2, 8);
        const int oct = (int)rnd(NLEVELS);
        MapPoint *p = new MapPoint();
        p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
        const float x = (u - Frame::cx) * z / Frame::fx, y = (v - Frame::cy) * z / Frame::fy, d = std::sqrt(x * x + y * y + z * z);
        p->mWorldPos.at<float>(0, 0) = x, p->mWorldPos.at<float>(1, 0) = y, p->mWorldPos.at<float>(2, 0) = z + 0.12f;
        p->mNormalVector.at<float>(0, 0) = 0, p->mNormalVector.at<float>(1, 0) = 0, p->mNormalVector.at<float>(2, 0) = -1;
        p->mfMaxDistance = d * powf(S, oct - 0.5f), p->mfMinDistance = p->mfMaxDistance / powf(S, NLEVELS - 1);
        p->nObs = rnd(5) ? 3 : 0;
        for (int b = 0; b < 32; b++) p->mDescriptor.ptr(0)[b] = (unsigned char)rnd(256);
        pts.push_back(p);
        const float ang = frand(0, 350);
        Cur.mvKeys.push_back(cv::KeyPoint(u + frand(-1, 1), v + frand(-1, 1), 31.f, ang + frand(0, 3), 50.f, oct, -1));
        Last.mvKeys.push_back(cv::KeyPoint(frand(4, W - 4), frand(4, H - 4), 31.f, ang, 50.f, oct, -1));
        Cur.mvuRight.push_back(rnd(10) < 7 ? Cur.mvKeys.back().pt.x - Cur.mbf / z : -1.f);
        memcpy(dc.ptr(i), p->mDescriptor.ptr(0), 32), memcpy(dl.ptr(i), p->mDescriptor.ptr(0), 32);
        for (int b = 0; b < 4; b++) dc.ptr(i)[rnd(32)] ^= (unsigned char)(1u << rnd(8));
    }
    Cur.N = Last.N = N;
    Cur.mvKeysUn = Cur.mvKeys, Last.mvKeysUn = Last.mvKeys;
    Cur.mDescriptors = dc, Last.mDescriptors = dl;
    Cur.mvpMapPoints.assign(N, (MapPoint *)NULL), Last.mvpMapPoints.assign(N, (MapPoint *)NULL);
    Cur.mvbOutlier.assign(N, false), Last.mvbOutlier.assign(N, false);
    KeyFrame kf;
    kf.N = N, kf.mvKeys = Last.mvKeys, kf.mvKeysUn = Last.mvKeysUn, kf.mDescriptors = dl.clone();
    kf.mnMinX = 0, kf.mnMaxX = W, kf.mnMinY = 0, kf.mnMaxY = H;
    kf.mfGridElementWidthInv = Frame::mfGridElementWidthInv, kf.mfGridElementHeightInv = Frame::mfGridElementHeightInv;
    kf.mnScaleLevels = NLEVELS, kf.mfScaleFactor = S, kf.mfLogScaleFactor = logf(S), kf.mvScaleFactors = Last.mvScaleFactors;
    kf.mvpMapPoints.assign(N, (MapPoint *)NULL);
    int held = 0;
    for (int i = 0; i < N; i++)
        if (rnd(10)) Last.mvpMapPoints[i] = kf.mvpMapPoints[i] = pts[i], pts[i]->AddObservation(&kf, i), held++;
    LS.Put(pts);
    LS.PutKeyFrame(&kf);
    std::set<MapPoint *> found;
    for (int i = 0; i < N; i += 7) found.insert(pts[i]);
    const uint64_t curKey = Cur.mnId + 1, lastKey = Last.mnId + 1, kfSetKey = (1ull << 62) | (kf.mnId + 1);

    ORBmatcher matcher(0.9f, true);
    std::vector<double> t[8];
    int nLast = -1, nKf = -1;
    for (int r = -10; r < reps; r++) {
        for (int mode = 0; mode < 8; mode++) {
            Frame F = Cur;
            const bool last = mode < 4;
            const int how = mode & 3;
            if (how == 2) {     // cold: the sets leave the device before the call (outside the timed window)
                orbhip_set_drop(LS.ctx(), curKey);
                orbhip_set_drop(LS.ctx(), last ? lastKey : kfSetKey);
            }
            const Clock::time_point t0 = Clock::now();
            int n;
            if (last)
                n = how == 0 ? matcher.SearchByProjection(F, Last, 7.f, false)
                  : how == 3 ? refpt::SearchLastFrame(F, Last, 7.f, false, true) : LS.SearchLastFrame(F, Last, 7.f, false);
            else
                n = how == 0 ? matcher.SearchByProjection(F, &kf, found, 10.f, 100)
                  : how == 3 ? refpt::SearchKeyFramePoints(F, &kf, found, 10.f, 100, true) : LS.SearchKeyFramePoints(F, &kf, found, 10.f, 100);
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            int &want = last ? nLast : nKf;
            static std::vector<MapPoint *> keepLast, keepKf;
            std::vector<MapPoint *> &keep = last ? keepLast : keepKf;
            if (want < 0) want = n, keep = F.mvpMapPoints;
            if (n != want || F.mvpMapPoints != keep) return printf("mode %d differs: %d matches against %d\n", mode, n, want), 1;
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    const char *names[8] = {"last_a_orbmatcher", "last_b_resident", "last_c_cold_sets", "last_d_host_loop",
                            "kf_a_orbmatcher", "kf_b_resident", "kf_c_cold_sets", "kf_d_host_loop"};
    for (int m = 0; m < 8; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape source %d frame %d held %d last_matches %d kf_matches %d\n", N, N, held, nLast, nKf);
    for (size_t i = 0; i < pts.size(); i++) delete pts[i];
    return 0;
}
