// fuse_latency.cpp -- the two Fuse loops of LocalMapping::SearchInNeighbors per call from a C++ caller, the path the library had
// before against the resident one (tools/fuse_latency.py runs it).  One new key frame of N features, most
// with a fresh map point, and K neighbours of N features over the same 6 N landmarks (each key frame detects N of them), holding
// older points of those landmarks.  Per repetition, on the same map restored each time, alternating in one process:
//   first pass: the new key frame's points into the K neighbours
//     a  ORBmatcher::Fuse called per target as it stands: every point read and projected on the host, queries and descriptors
//        uploaded per call (the parent's path; ORBmatcher is unchanged)
//     b  LocalMapSearch::FuseInTargets with points, rows and feature sets resident, the resident state kept up to date
//     c  the same with the feature sets dropped before the call (put cold inside it)
//     d  the reference's loop restated on the host with the oracle's window search on one core (tests/native_fuse/ref_fuse.h)
//   second pass, on the map the first pass left: the neighbours' points (the first C of them, ~5 N candidates) into the new key frame
//     a  the candidate list built on the host, then ORBmatcher::Fuse      b / c  LocalMapSearch::FuseCandidates      d  the host loop
// a, b, c and d must return the same counts and leave the same map (rows, bad flags, observation counts), or the program fails.
// usage: fuse_latency N K C reps      prints "<name> median <us> p10 <us> p90 <us>" lines, "floor <us>" (orbhip_debug_roundtrip
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
#include "ref_fuse.h"

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
static const float S = 1.2f, FX = 458.f, CX = 376.f, CY = 240.f, MBF = 40.f;

static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;
static std::vector<MapPoint> g_savedPts;                    // the map as built: restored before every timed call of the first pass
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

static void build(int N, int K)
{
    const int NLM = 6 * N;
    std::vector<float> P((size_t)NLM * 3);
    std::vector<unsigned char> D((size_t)NLM * 32);
    for (int j = 0; j < NLM; j++) {
        const float z = frand(3, 12);
        P[3 * j] = (frand(20, W - 20) - CX) * z / FX, P[3 * j + 1] = (frand(20, H - 20) - CY) * z / FX, P[3 * j + 2] = z;
        for (int b = 0; b < 32; b++) D[(size_t)j * 32 + b] = (unsigned char)rnd(256);
    }
    std::vector<MapPoint *> oldOf(NLM, (MapPoint *)NULL);
    for (int k = 0; k <= K; k++) {
        KeyFrame *kf = new KeyFrame();
        g_kfs.push_back(kf);
        const float C[3] = {0.004f * k, 0.002f * (k % 5), 0.003f * (k % 7)};   // the neighbourhood of one place
        kf->Tcw = cv::Mat::zeros(4, 4, CV_32F), kf->Ow = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) kf->Tcw.at<float>(r, r) = 1.f, kf->Tcw.at<float>(r, 3) = -C[r], kf->Ow.at<float>(r, 0) = C[r];
        kf->Tcw.at<float>(3, 3) = 1.f;
        kf->fx = kf->fy = FX, kf->cx = CX, kf->cy = CY, kf->mbf = MBF;
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
            kf->mvuRight.push_back(rnd(10) < 7 ? u - MBF / z + frand(-0.3f, 0.3f) : -1.f);
            unsigned char *d = kf->mDescriptors.ptr(i);
            memcpy(d, &D[(size_t)j * 32], 32);
            for (int b = 0; b < 6; b++) d[rnd(32)] ^= (unsigned char)(1u << rnd(8));
            if (k == 0) {                          // the new key frame: a fresh point on 8 features in 10
                if (rnd(10) < 8) {
                    MapPoint *p = new_point(&P[3 * j], d);
                    kf->mvpMapPoints[i] = p, p->AddObservation(kf, i);
                }
            } else if (rnd(10) < 7) {              // a neighbour: the landmark's older point, unless it is in this key frame already
                if (!oldOf[j]) oldOf[j] = new_point(&P[3 * j], d);
                if (!oldOf[j]->IsInKeyFrame(kf)) kf->mvpMapPoints[i] = oldOf[j], oldOf[j]->AddObservation(kf, i);
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

static unsigned long long digest(const std::vector<int> &counts)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < counts.size(); i++) h = (h ^ (unsigned long long)counts[i]) * 1099511628211ull;
    for (size_t k = 0; k < g_kfs.size(); k++)
        for (size_t i = 0; i < g_kfs[k]->mvpMapPoints.size(); i++)
            h = (h ^ (g_kfs[k]->mvpMapPoints[i] ? g_kfs[k]->mvpMapPoints[i]->mnId + 1 : 0)) * 1099511628211ull;
    for (size_t i = 0; i < g_pts.size(); i++) h = (h ^ ((unsigned long long)g_pts[i]->Observations() * 2 + (g_pts[i]->isBad() ? 1 : 0))) * 1099511628211ull;
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
    const int N = argc > 1 ? atoi(argv[1]) : 1000, K = argc > 2 ? atoi(argv[2]) : 10, C = argc > 3 ? atoi(argv[3]) : 8,
              reps = argc > 4 ? atoi(argv[4]) : 20;
    if (N < 16 || N > 8192 || K < 1 || C < 1 || C > K) return printf("usage: fuse_latency N K C reps (C <= K)\n"), 2;
    MapPoint::RecomputeOnReplace() = true;         // Replace ends in ComputeDistinctiveDescriptors, as in the reference
    build(N, K);
    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(K + 8, N);
    KeyFrame *cur = g_kfs[0];
    const std::vector<KeyFrame *> targets(g_kfs.begin() + 1, g_kfs.end()), some(g_kfs.begin() + 1, g_kfs.begin() + 1 + C);

    ORBmatcher matcher;
    std::vector<double> t[8];
    unsigned long long want1 = 0, want2 = 0;
    long fused1 = 0, fused2 = 0, ncand = 0;
    for (int r = -3; r < reps; r++) {
        for (int mode = 0; mode < 4; mode++) {
            const bool resident = mode == 1 || mode == 2;
            restore(resident ? &LS : NULL);
            if (mode == 2) orbhip_set_drop(LS.ctx(), 0);        // cold: the sets leave the device before the call (not timed)
            std::vector<int> n1;
            Clock::time_point t0 = Clock::now();
            if (mode == 0) {
                const std::vector<MapPoint *> vp = cur->GetMapPointMatches();
                for (size_t k = 0; k < targets.size(); k++) n1.push_back(matcher.Fuse(targets[k], vp));
            } else if (mode == 3)
                n1 = reffuse::FuseInTargets(cur, targets, 3.0f);
            else
                n1 = LS.FuseInTargets(cur, targets);
            double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            const unsigned long long d1 = digest(n1);
            if (!want1) {
                want1 = d1;
                for (size_t k = 0; k < n1.size(); k++) fused1 += n1[k];
            }
            if (d1 != want1) return printf("first pass, mode %d: another result\n", mode), 1;
            if (mode == 2) orbhip_set_drop(LS.ctx(), 0);
            int n2;
            t0 = Clock::now();
            if (mode == 0) {
                const std::vector<MapPoint *> cand = reffuse::Candidates(some);
                ncand = (long)cand.size();
                n2 = matcher.Fuse(cur, cand);
            } else if (mode == 3)
                n2 = reffuse::FuseCandidates(cur, some, 3.0f);
            else
                n2 = LS.FuseCandidates(cur, some);
            us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[4 + mode].push_back(us);
            const unsigned long long d2 = digest(std::vector<int>(1, n2));
            if (!want2) want2 = d2, fused2 = n2;
            if (d2 != want2) return printf("second pass, mode %d: another result\n", mode), 1;
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    const char *names[8] = {"targets_a_orbmatcher", "targets_b_resident", "targets_c_cold_sets", "targets_d_host_loop",
                            "candidates_a_orbmatcher", "candidates_b_resident", "candidates_c_cold_sets", "candidates_d_host_loop"};
    for (int m = 0; m < 8; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape features %d targets %d fused_in_targets %ld candidate_kfs %d candidates %ld fused_candidates %ld points %d\n", N, K, fused1, C,
           ncand, fused2, (int)g_pts.size());
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
