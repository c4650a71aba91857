// sim3search_latency.cpp -- ORBmatcher::SearchBySim3 per call from a C++ caller, the path the library had before against the
// resident one (tools/sim3search_latency.py runs it).  The two sides of a loop: two key frames of N features
// that see the same landmarks through a similarity of scale 1.37; about 60 % of the entries of each hold a point of their own map,
// every ninth landmark that both hold is matched beforehand, as SearchByBoW leaves it.  Per repetition, on the same objects,
// alternating in one process:
//   a  ORBmatcher::SearchBySim3 (the parent's path; ORBmatcher is unchanged): two host projections, two orbhip_window_best_set
//      calls, the agreement on the host
//   b  LocalMapSearch::SearchBySim3 with points, rows and feature sets resident: taken bytes, one orbhip_search_by_sim3, pointers
//   c  orbhip_search_by_sim3 alone, its arguments prepared once
// a and b must return the same number and leave the same vpMatches12, or the program fails.
// usage: sim3search_latency N reps      prints "<name> median <us> p10 <us> p90 <us>" lines, "floor <us>" (orbhip_debug_roundtrip
// mode 1 on the searching context) and "shape ..."
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "LocalMapDetail.h"
#include "MatcherDetail.h"
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
static const float S = 1.2f, FX = 458.f, CX = 376.f, CY = 240.f, S12 = 1.37f;

static KeyFrame *g_kf[2];
static std::vector<MapPoint *> g_pts, g_before;
static cv::Mat g_R12, g_t12;

static MapPoint *new_point(const float P[3], const unsigned char *desc)
{
    MapPoint *p = new MapPoint();
    p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
    for (int k = 0; k < 3; k++) p->mWorldPos.at<float>(k, 0) = P[k], p->mNormalVector.at<float>(k, 0) = k == 2 ? 1.f : 0.f;
    memcpy(p->mDescriptor.ptr(0), desc, 32);
    p->mfMaxDistance = 12.f, p->mfMinDistance = 12.f / powf(S, NLEVELS - 1);
    g_pts.push_back(p);
    return p;
}

static void build(int N)
{
    const float a = 0.02f, R[9] = {cosf(a), 0, sinf(a), 0, 1, 0, -sinf(a), 0, cosf(a)}, t[3] = {0.15f, -0.05f, 0.3f};
    g_R12 = cv::Mat(3, 3, CV_32F), g_t12 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) g_R12.at<float>(r, c) = R[3 * r + c];
        g_t12.at<float>(r, 0) = t[r];
    }
    for (int k = 0; k < 2; k++) {
        KeyFrame *kf = g_kf[k] = new KeyFrame();
        const float C[3] = {0.3f * k, 0.05f * k, 0.1f * k};
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
    }
    g_before.assign(N, (MapPoint *)NULL);
    for (int i = 0; i < N; i++) {
        unsigned char base[32];
        for (int b = 0; b < 32; b++) base[b] = (unsigned char)rnd(256);
        // the landmark in camera 1 and, through the similarity, in camera 2: p2 = (1 / s12) R12' (p1 - t12)
        double pc[2][3];
        for (;;) {
            const double z = frand(3.5f, 11.f);
            pc[0][0] = (frand(20, W - 20) - CX) * z / FX, pc[0][1] = (frand(20, H - 20) - CY) * z / FX, pc[0][2] = z;
            for (int r = 0; r < 3; r++) {
                double s = 0;
                for (int q = 0; q < 3; q++) s += (double)R[3 * q + r] * (pc[0][q] - (double)t[q]);
                pc[1][r] = s / (double)S12;
            }
            const double u2 = FX * pc[1][0] / pc[1][2] + CX, v2 = FX * pc[1][1] / pc[1][2] + CY;
            if (u2 > 4 && u2 < W - 4 && v2 > 4 && v2 < H - 4) break;
        }
        MapPoint *both[2] = {NULL, NULL};
        for (int k = 0; k < 2; k++) {
            KeyFrame *kf = g_kf[k];
            const float u = FX * (float)(pc[k][0] / pc[k][2]) + CX + frand(-0.5f, 0.5f), v = FX * (float)(pc[k][1] / pc[k][2]) + CY + frand(-0.5f, 0.5f);
            const float dist = (float)sqrt(pc[k][0] * pc[k][0] + pc[k][1] * pc[k][1] + pc[k][2] * pc[k][2]);
            int oct = (int)floorf(logf(12.f / dist) / logf(S));
            oct = oct < 0 ? 0 : oct > NLEVELS - 1 ? NLEVELS - 1 : oct;
            kf->mvKeys.push_back(cv::KeyPoint(u, v, 31.f * powf(S, (float)oct), frand(0, 360), 50.f, oct, -1));
            unsigned char *d = kf->mDescriptors.ptr(i);
            memcpy(d, base, 32);
            for (int b = 0; b < 6; b++) d[rnd(32)] ^= (unsigned char)(1u << rnd(8));
            if (rnd(10) < 6) {
                float P[3];
                for (int r = 0; r < 3; r++) P[r] = (float)(pc[k][r] + (double)kf->Ow.at<float>(r, 0));   // (the poses are translations)
                both[k] = new_point(P, d);
                kf->mvpMapPoints[i] = both[k], both[k]->AddObservation(kf, i);
            }
        }
        if (i % 9 == 0 && both[0] && both[1]) g_before[i] = both[1];
    }
    for (int k = 0; k < 2; k++) g_kf[k]->mvKeysUn = g_kf[k]->mvKeys, g_kf[k]->N = N;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int N = argc > 1 ? atoi(argv[1]) : 1000, reps = argc > 2 ? atoi(argv[2]) : 20;
    if (N < 16 || N > 8192 || reps < 1) return printf("usage: sim3search_latency N reps\n"), 2;
    build(N);
    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(8, N);
    LS.Put(g_pts);
    LS.PutKeyFrame(g_kf[0]);
    LS.PutKeyFrame(g_kf[1]);
    const float th = 7.5f;                               // ref: src/LoopClosing.cc:375
    ORBmatcher matcher(0.75f, true);                     // ref: src/LoopClosing.cc:246
    std::vector<double> t[3];
    std::vector<MapPoint *> want;
    int nWant = -2;
    // c: the entry point's arguments, prepared once (the resident sets are those of b: it runs first)
    orbhip_fuse_target sides[2];
    uint64_t rowKeys[2];
    float r12[9], r21[9], t12v[3], t21[3];
    std::vector<uint8_t> taken1(N, 0), taken2(N, 0);
    std::vector<int32_t> match12(N);
    for (int r = -2; r < reps; r++) {
        for (int mode = 0; mode < 2; mode++) {
            std::vector<MapPoint *> m = g_before;
            const Clock::time_point t0 = Clock::now();
            const int n = mode == 0 ? matcher.SearchBySim3(g_kf[0], g_kf[1], m, S12, g_R12, g_t12, th)
                                    : LS.SearchBySim3(g_kf[0], g_kf[1], m, S12, g_R12, g_t12, th);
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            if (nWant == -2) nWant = n, want = m;
            if (n != nWant || m != want) return printf("SearchBySim3, mode %d: another result (%d, %d)\n", mode, n, nWant), 1;
        }
        if (r == -2) {
            cv::Mat sR12, sR21;
            hipdetail::scale3(g_R12, (double)S12, false, sR12);
            hipdetail::scale3(g_R12, 1.0 / S12, true, sR21);
            for (int i = 0; i < 3; i++) {
                t12v[i] = g_t12.at<float>(i, 0);
                for (int c = 0; c < 3; c++) r12[3 * i + c] = sR12.at<float>(i, c), r21[3 * i + c] = sR21.at<float>(i, c);
            }
            hipdetail::affine3(sR21, t12v, NULL, t21, false, -1.0);
            for (int s = 0; s < 2; s++) {
                localmapdetail::fill_target(g_kf[s], localmapdetail::set_key_of(g_kf[s]), th, &sides[s]);
                rowKeys[s] = localmapdetail::key_of(g_kf[s]);
            }
            for (int i = 0; i < N; i++)
                if (g_before[i]) {
                    taken1[i] = 1;
                    const int idx2 = g_before[i]->GetIndexInKeyFrame(g_kf[1]);
                    if (idx2 >= 0 && idx2 < N) taken2[idx2] = 1;
                }
        }
        int nf = 0;
        int32_t na[2];
        const Clock::time_point t0 = Clock::now();
        const int rc = orbhip_search_by_sim3(LS.ctx(), sides, rowKeys, r21, t21, r12, t12v, th, 100, taken1.data(), taken2.data(), match12.data(), &nf,
                                             na, NULL, NULL, NULL, NULL, NULL, NULL);
        const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
        if (r >= 0) t[2].push_back(us);
        if (rc != ORBHIP_OK || nf != nWant) return printf("orbhip_search_by_sim3: rc %d, %d found, %d wanted\n", rc, nf, nWant), 1;
    }
    if (nWant < 0) return printf("LocalMapSearch::SearchBySim3 sent the pair the host way\n"), 1;
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    const char *names[3] = {"sim3_a_orbmatcher", "sim3_b_resident", "sim3_c_entry"};
    for (int m = 0; m < 3; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    int before = 0;
    for (int i = 0; i < N; i++) before += g_before[i] ? 1 : 0;
    printf("shape features %d points %d matched_before %d found %d\n", N, (int)g_pts.size(), before, nWant);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    delete g_kf[0];
    delete g_kf[1];
    return 0;
}
