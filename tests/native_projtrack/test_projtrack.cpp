// test_projtrack.cpp -- ORB_SLAM2::LocalMapSearch::SearchLastFrame and ::SearchKeyFramePoints over a sequence of frames, on mock
// Frame / KeyFrame / MapPoint objects: a camera moving along its axis past a cloud of landmarks, with temporal points that never
// entered the store, a point that turns bad, points that are erased and whose slots go to new points, key frames whose rows go
// stale.  Every call is compared with a reference on a copy of the same frame:
//   -DPROJTRACK_MOCK  the class runs on the host model of the entry points (mock_projtrack.cc), the reference is the restatement
//                     of the two loops on the objects themselves (ref_projtrack.h); no device, no liborbhip
//   otherwise         the class runs on liborbhip, the reference is ORBmatcher's two methods (the path before these entry points)
// Prints "ok <frames> <calls> <matches> <digest>" and returns 0, or the failed checks.  The digest is over every return value and
// every match, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#ifdef PROJTRACK_MOCK
#include "ref_projtrack.h"
#else
#include "ORBmatcher.h"
#endif

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 2024;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 16) / 65536.f; }

static const int W = 376, H = 241, NLEVELS = 8, NLM = 520;
static const float S = 1.2f;

struct Landmark {
    float P[3], angle;
    uint8_t desc[32];
    MapPoint *mp;
};
static std::vector<Landmark> g_lm;
static std::vector<MapPoint *> g_all;

static MapPoint *new_point(const Landmark &L, float maxDist)
{
    MapPoint *p = new MapPoint();
    p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
    for (int k = 0; k < 3; k++) p->mWorldPos.at<float>(k, 0) = L.P[k], p->mNormalVector.at<float>(k, 0) = k == 2 ? -1.f : 0.f;
    memcpy(p->mDescriptor.ptr(0), L.desc, 32);
    p->mfMaxDistance = maxDist, p->mfMinDistance = maxDist / powf(S, NLEVELS - 1);
    g_all.push_back(p);
    return p;
}

static cv::Mat pose(int t, float err)
{
    cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
    const float a = 0.004f * t + err, c = cosf(a), s = sinf(a);
    const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    const float C[3] = {0.02f * t + err, 0.3f * err, 0.15f * t};     // moves along its axis by more than the baseline per frame
    for (int r = 0; r < 3; r++) {
        float tr = 0;
        for (int k = 0; k < 3; k++) T.at<float>(r, k) = R[3 * r + k], tr -= R[3 * r + k] * C[k];
        T.at<float>(r, 3) = tr;
    }
    T.at<float>(3, 3) = 1.f;
    return T;
}

struct Shot {
    Frame F;
    std::vector<int> lm;   // landmark of each feature, -1 = clutter
};

static void make_frame(Shot &sh, int t, float err)
{
    Frame &F = sh.F;
    F.mTcw = pose(t, err);
    F.mnScaleLevels = NLEVELS, F.mfScaleFactor = S, F.mfLogScaleFactor = logf(S);
    for (int l = 0; l < NLEVELS; l++) F.mvScaleFactors.push_back(powf(S, (float)l));
    F.mbf = 40.f, F.mb = 0.08f;
    std::vector<uint8_t> rows;
    const cv::Mat T0 = pose(t, 0.f);   // the features are where the camera really is; F.mTcw is the prediction
    for (int j = 0; j < NLM + 80; j++) {
        cv::KeyPoint kp;
        uint8_t d[32];
        float z = 0;
        if (j < NLM) {
            const Landmark &L = g_lm[j];
            float pc[3];
            for (int r = 0; r < 3; r++) pc[r] = T0.at<float>(r, 0) * L.P[0] + T0.at<float>(r, 1) * L.P[1] + T0.at<float>(r, 2) * L.P[2] + T0.at<float>(r, 3);
            if (pc[2] < 0.5f) continue;
            const float u = Frame::fx * pc[0] / pc[2] + Frame::cx + frand(-0.6f, 0.6f), v = Frame::fy * pc[1] / pc[2] + Frame::cy + frand(-0.6f, 0.6f);
            if (u < 1 || u > W - 2 || v < 1 || v > H - 2) continue;
            z = pc[2];
            int oct = (int)floorf(logf(12.f / z) / logf(S));
            oct = oct < 0 ? 0 : oct > NLEVELS - 1 ? NLEVELS - 1 : oct;
            kp = cv::KeyPoint(u, v, 31.f * powf(S, (float)oct), fmodf(L.angle + frand(0, 4) + (rnd(25) == 0 ? 120.f : 0.f), 360.f), 50.f, oct, -1);
            memcpy(d, L.desc, 32);
            for (int b = 0; b < 4; b++) d[rnd(32)] ^= (uint8_t)(1u << rnd(8));
        } else {
            kp = cv::KeyPoint(frand(1, W - 2), frand(1, H - 2), 31.f, frand(0, 360), 20.f, (int)rnd(NLEVELS), -1);
            for (int b = 0; b < 32; b++) d[b] = (uint8_t)rnd(256);
        }
        F.mvKeys.push_back(kp);
        F.mvuRight.push_back(z > 0 && rnd(10) < 7 ? kp.pt.x - F.mbf / z + frand(-0.3f, 0.3f) : -1.f);
        rows.insert(rows.end(), d, d + 32);
        sh.lm.push_back(j < NLM ? j : -1);
    }
    F.mvKeysUn = F.mvKeys;
    F.N = (int)F.mvKeys.size();
    F.mDescriptors = cv::Mat(F.N, 32, CV_8U);
    memcpy(F.mDescriptors.ptr(0), rows.data(), rows.size());
    F.mvpMapPoints.assign(F.N, (MapPoint *)NULL);
    F.mvbOutlier.assign(F.N, false);
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

static long g_calls = 0, g_matches = 0;
static void compare(const Frame &A, const Frame &B, int nA, int nB)
{
    CHECK(nA == nB);
    CHECK(A.mvpMapPoints == B.mvpMapPoints);
    g_calls++, g_matches += nA;
    mix((unsigned long long)nA);
    for (int i = 0; i < A.N; i++) mix(A.mvpMapPoints[i] ? A.mvpMapPoints[i]->mnId + 1 : 0);
}

static int ref_last(Frame &Cur, const Frame &Last, float th, bool mono)
{
#ifdef PROJTRACK_MOCK
    return refpt::SearchLastFrame(Cur, Last, th, mono, true);
#else
    ORBmatcher matcher(0.9f, true);     // ref: src/Tracking.cc, TrackWithMotionModel
    return matcher.SearchByProjection(Cur, Last, th, mono);
#endif
}

static int ref_kf(Frame &Cur, KeyFrame *kf, const std::set<MapPoint *> &found, float th, int dist)
{
#ifdef PROJTRACK_MOCK
    return refpt::SearchKeyFramePoints(Cur, kf, found, th, dist, true);
#else
    ORBmatcher matcher(0.9f, true);     // ref: src/Tracking.cc, Relocalization (matcher2)
    return matcher.SearchByProjection(Cur, kf, found, th, dist);
#endif
}

int main()
{
    Frame::fx = 300, Frame::fy = 300, Frame::cx = 188, Frame::cy = 120.5f;
    Frame::mnMinX = 0, Frame::mnMaxX = W, Frame::mnMinY = 0, Frame::mnMaxY = H;
    Frame::mfGridElementWidthInv = (float)FRAME_GRID_COLS / W, Frame::mfGridElementHeightInv = (float)FRAME_GRID_ROWS / H;
    LocalMapSearch LS(2048);
    LS.InitKeyFrames(8, 1024);

    g_lm.resize(NLM);
    std::vector<MapPoint *> first;
    for (int j = 0; j < NLM; j++) {
        Landmark &L = g_lm[j];
        L.P[0] = frand(-4, 4), L.P[1] = frand(-2.5f, 2.5f), L.P[2] = frand(3, 12), L.angle = frand(0, 350);
        for (int b = 0; b < 32; b++) L.desc[b] = (uint8_t)rnd(256);
        L.mp = new_point(L, j % 17 == 0 ? 2.f : 12.f);       // every 17th is out of its distance range for the key-frame form
        L.mp->nObs = j % 5 == 0 ? 0 : 3;                     // some have no observations yet: they do not close a feature
        first.push_back(L.mp);
    }
    LS.Put(first);

    const int T = 9;
    std::vector<Shot> shots(T);
    for (int t = 0; t < T; t++) make_frame(shots[t], t, t == 0 ? 0.f : frand(-0.004f, 0.004f));
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> temporal;
    int nBad = 0, nReused = 0, nStale = 0, nTemporal = 0;

    for (int t = 1; t < T; t++) {
        // ---- the last frame as tracking left it: its landmarks' points, a few outliers, temporal points for some of the rest ----
        Shot &last = shots[t - 1];
        Frame &Last = last.F;
        for (int i = 0; i < Last.N; i++) {
            const int j = last.lm[i];
            Last.mvpMapPoints[i] = NULL, Last.mvbOutlier[i] = false;
            if (j < 0) continue;
            const unsigned r = rnd(100);
            if (r < 72) Last.mvpMapPoints[i] = g_lm[j].mp;
            else if (r < 80) {                               // UpdateLastFrame's temporal point: never Put, no observations
                MapPoint *p = new_point(g_lm[j], 12.f);
                temporal.push_back(p), nTemporal++;
                Last.mvpMapPoints[i] = p;
            }
            if (Last.mvpMapPoints[i] && rnd(20) == 0) Last.mvbOutlier[i] = true;
        }
        // ---- the map changes between frames ----
        if (t == 3 || t == 6)
            for (int k = 0; k < 12; k++) {                   // points turn bad: still searched from the last frame, not from a key frame
                MapPoint *p = g_lm[rnd(NLM)].mp;
                p->SetBadFlag();
                LS.UpdateFlags(p), nBad++;
            }
        if (t == 4 || t == 7)
            for (int k = 0; k < 15; k++) {                   // points leave the map; new ones take their landmarks (and their slots)
                Landmark &L = g_lm[rnd(NLM)];
                MapPoint *old = L.mp;
                for (size_t f = 0; f < kfs.size(); f++)
                    for (size_t i = 0; i < kfs[f]->mvpMapPoints.size(); i++)
                        if (kfs[f]->mvpMapPoints[i] == old) {
                            kfs[f]->EraseMapPointMatch(i);                   // SetBadFlag's EraseMapPointMatch
                            if (k & 1) LS.SetMapPoint(kfs[f], i, NULL);      // told, or left to go stale in the table
                            else nStale++;
                        }
                for (int i = 0; i < Last.N; i++)
                    if (Last.mvpMapPoints[i] == old) Last.mvpMapPoints[i] = NULL;
                LS.Erase(old);
                L.mp = new_point(L, 12.f);
                L.mp->nObs = 2;
                LS.Put(L.mp), nReused++;
            }
        // ---- TrackWithMotionModel's search, stereo and monocular, narrow and wide ----
        for (int variant = 0; variant < 3; variant++) {
            const bool mono = variant == 1;
            const float th = variant == 2 ? 14.f : mono ? 15.f : 7.f;
            Frame A = shots[t].F, B = shots[t].F;
            if (mono) A.mvuRight.clear(), B.mvuRight.clear();
            for (int i = 0; i < A.N; i += 23)                // features that already hold a point: closed when it has observations
                A.mvpMapPoints[i] = B.mvpMapPoints[i] = g_lm[(i * 7) % NLM].mp;
            const int nA = LS.SearchLastFrame(A, Last, th, mono), nB = ref_last(B, Last, th, mono);
            compare(A, B, nA, nB);
            if (variant == 0) CHECK(nA >= 100);
            // ---- Relocalization's search against every key frame so far, with what the first search found as sAlreadyFound ----
            for (size_t f = 0; f < kfs.size() && variant == 0; f++) {
                std::set<MapPoint *> found;
                for (int i = 0; i < A.N; i += 2)
                    if (A.mvpMapPoints[i]) found.insert(A.mvpMapPoints[i]);
                Frame A2 = shots[t].F, B2 = shots[t].F;
                for (int i = 0; i < A2.N; i += 3) A2.mvpMapPoints[i] = B2.mvpMapPoints[i] = A.mvpMapPoints[i];
                const int mA = LS.SearchKeyFramePoints(A2, kfs[f], found, 10.f, t & 1 ? 100 : 64);
                const int mB = ref_kf(B2, kfs[f], found, 10.f, t & 1 ? 100 : 64);
                compare(A2, B2, mA, mB);
                CHECK(mA >= 20);
            }
        }
        for (size_t k = 0; k < temporal.size(); k++) LS.Erase(temporal[k]);      // Tracking deletes its temporal points
        temporal.clear();
        // ---- the last frame becomes a key frame now and then ----
        if (t == 2 || t == 5) {
            KeyFrame *kf = new KeyFrame();
            kf->N = Last.N;
            kf->mvKeys = Last.mvKeys, kf->mvKeysUn = Last.mvKeysUn, kf->mDescriptors = Last.mDescriptors.clone();
            kf->mvuRight = Last.mvuRight;
            kf->mnMinX = 0, kf->mnMaxX = W, kf->mnMinY = 0, kf->mnMaxY = H;
            kf->mfGridElementWidthInv = Frame::mfGridElementWidthInv, kf->mfGridElementHeightInv = Frame::mfGridElementHeightInv;
            kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = S, kf->mfLogScaleFactor = logf(S), kf->mvScaleFactors = Last.mvScaleFactors;
            kf->mvpMapPoints.assign(kf->N, (MapPoint *)NULL);
            std::vector<MapPoint *> seen;
            for (int i = 0; i < kf->N; i++) {
                const int j = last.lm[i];
                if (j < 0 || rnd(10) == 0) continue;
                MapPoint *p = g_lm[j].mp;
                kf->mvpMapPoints[i] = p;
                p->AddObservation(kf, i);
                seen.push_back(p);
            }
            LS.Put(seen);                                    // their observation counts changed
            if (t == 2) LS.PutKeyFrame(kf);                  // (the second one is put by its first search)
            kfs.push_back(kf);
        }
    }
    CHECK(nBad >= 20 && nReused >= 25 && nStale >= 1 && nTemporal >= 100 && kfs.size() == 2);
    CHECK(OrbHipErrorCount() == 0);
    for (size_t i = 0; i < g_all.size(); i++) delete g_all[i];
    for (size_t f = 0; f < kfs.size(); f++) delete kfs[f];
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %ld %ld %016llx\n", T - 1, g_calls, g_matches, g_digest);
    return 0;
}
