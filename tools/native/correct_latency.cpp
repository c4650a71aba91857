// correct_latency.cpp -- what CorrectLoop's Sim3 pass and the global-BA update cost a C++ caller (tools/correct_latency.py; DESIGN.md
// section 23): a map of NKF key frames of NF features, every point seen from about five of them, K key frames corrected.
//   loop_a_host_put  the reference's loop on slamlite.h objects (tests/native_correct/ref_correct.h), then LocalMapSearch::Put of the
//                    points it moved: the path of the parent commit
//   loop_b_correct   LocalMapSearch::CorrectLoopPoints: one orbhip_map_correct_sim3 call on the resident store
//   loop_b_entry     the entry point alone, inside b (LocalMapSearch::CorrectTimes().device)
//   gba_a_host_put   the reference's global-BA point loop over the whole map, then Put of the points it moved
//   gba_b_apply      LocalMapSearch::ApplyGlobalBA: one orbhip_map_correct_se3 call
//   gba_b_entry      the entry point alone, inside b
// Before every timed call the objects and the store are put back to the same values (not timed).  The program fails unless a and b
// leave the same positions, normals, ranges and poses.  Prints "<mode> median <us> p10 <us> p90 <us>" per mode, "floor <us>"
// (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "correct_poses.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_correct.h"

typedef std::chrono::steady_clock Clock;

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;
static std::vector<MapPoint> g_saved;
static std::vector<Pose> g_poses;
static std::vector<cv::Mat> g_Tcw;

static void build(int NKF, int NF)
{
    g_seed = 2025;
    const int NLEVELS = 8, NPT = NKF * NF / 6;
    std::vector<int> nextFree(NKF, 0);
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        g_kfs.push_back(kf);
        g_poses.push_back(random_pose());
        g_Tcw.push_back(as_se3(g_poses[k]));
        kf->N = NF;
        kf->SetPose(g_Tcw[k]);
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = 1.2f, kf->mfLogScaleFactor = logf(1.2f);
        float s = 1.f;
        for (int l = 0; l < NLEVELS; l++, s *= 1.2f) kf->mvScaleFactors.push_back(s), kf->mvInvLevelSigma2.push_back(1.f / (s * s));
        for (int i = 0; i < NF; i++) kf->mvKeys.push_back(cv::KeyPoint((float)drand(2, 637), (float)drand(2, 477), 31.f, 0.f, 20.f, (int)rnd(NLEVELS), -1));
        kf->mvKeysUn = kf->mvKeys;
        kf->mvpMapPoints.assign(NF, (MapPoint *)NULL);
    }
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new MapPoint();
        p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c, 0) = (float)drand(-6, 6) + (c == 2 ? 9.f : 0.f), p->mNormalVector.at<float>(c, 0) = 0.f;
        for (int b = 0; b < 32; b++) p->mDescriptor.ptr(0)[b] = (uint8_t)rnd(256);
        p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
        // neighbouring key frames share points, as along a trajectory: 3 to 7 observers within a window of 12
        const int n = 3 + (int)rnd(5), first = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 100; tries++) {
            const int k = (first + (int)rnd(12)) % NKF;
            KeyFrame *kf = g_kfs[k];
            if (p->IsInKeyFrame(kf) || nextFree[k] >= kf->N) continue;
            const int idx = nextFree[k]++;
            kf->mvpMapPoints[idx] = p;
            p->AddObservation(kf, idx);
            if (!p->mpRefKF) p->mpRefKF = kf;
        }
        if (p->mObservations.empty()) {   // (its window of key frames is full)
            delete p;
            continue;
        }
        g_pts.push_back(p);
        cv::Mat g(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) g.at<float>(c, 0) = p->mWorldPos.at<float>(c, 0) + (float)drand(-0.1, 0.1);
        p->mPosGBA = g;
    }
    for (size_t i = 0; i < g_pts.size(); i++) g_saved.push_back(*g_pts[i]);
}

static unsigned long long digest()
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < g_pts.size(); i++) {
        MapPoint *p = g_pts[i];
        unsigned u[8];
        for (int c = 0; c < 3; c++) memcpy(&u[c], &p->mNormalVector.at<float>(c, 0), 4), memcpy(&u[3 + c], &p->mWorldPos.at<float>(c, 0), 4);
        memcpy(&u[6], &p->mfMinDistance, 4), memcpy(&u[7], &p->mfMaxDistance, 4);
        for (int c = 0; c < 8; c++) h = (h ^ u[c]) * 1099511628211ull;
    }
    for (size_t k = 0; k < g_kfs.size(); k++)
        for (int c = 0; c < 3; c++) {
            unsigned u;
            memcpy(&u, &g_kfs[k]->Ow.at<float>(c, 0), 4);
            h = (h ^ u) * 1099511628211ull;
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
    const int K = argc > 1 ? atoi(argv[1]) : 20, reps = argc > 2 ? atoi(argv[2]) : 15, NKF = argc > 3 ? atoi(argv[3]) : 200,
              NF = argc > 4 ? atoi(argv[4]) : 1000;
    if (K < 1 || K > NKF || reps < 1 || NKF < 13 || NF < 10) return printf("usage: correct_latency K reps [key_frames features]\n"), 2;
    build(NKF, NF);
    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    const unsigned long CURRENT_ID = 4242, LOOP_KF = 77;

    // the K corrected key frames: the current key frame's neighbourhood, consecutive along the trajectory, in ascending mnId
    g_seed = 99;
    std::vector<LoopCorrection> corr;
    const int first = NKF - K;
    for (int j = 0; j < K; j++) {
        const Pose corrected = nudged(g_poses[first + j], drand(0.9, 1.1));
        LoopCorrection L;
        L.pKF = g_kfs[first + j];
        L.Siw = as_sim3(g_poses[first + j]);
        L.correctedSwi = inverse(corrected);
        L.correctedTiw = as_se3(corrected);
        corr.push_back(L);
    }
    std::vector<MapPoint *> loopPoints;   // what the loop will move: for the Put of mode a (gathered outside the timed part)
    std::set<MapPoint *> seen;
    for (int j = 0; j < K; j++)
        for (size_t i = 0; i < corr[j].pKF->mvpMapPoints.size(); i++) {
            MapPoint *p = corr[j].pKF->mvpMapPoints[i];
            if (p && seen.insert(p).second) loopPoints.push_back(p);
        }
    long nobs = 0;
    for (size_t i = 0; i < loopPoints.size(); i++) nobs += (long)loopPoints[i]->mObservations.size();

    std::vector<double> t[6];
    unsigned long long want = 0;
    for (int r = -2; r < reps; r++)
        for (int mode = 0; mode < 2; mode++) {
            for (size_t i = 0; i < g_pts.size(); i++) *g_pts[i] = g_saved[i];
            for (int k = 0; k < NKF; k++) g_kfs[k]->SetPose(g_Tcw[k]);
            LS.Put(g_pts);
            LocalMapSearch::CorrectTimes().device = 0;
            const Clock::time_point t0 = Clock::now();
            if (mode == 0) {
                refcorrect::correct_loop(corr, CURRENT_ID);
                LS.Put(loopPoints);
            } else {
                LS.CorrectLoopPoints(corr, CURRENT_ID);
            }
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            if (r >= 0 && mode == 1) t[2].push_back(LocalMapSearch::CorrectTimes().device);
            const unsigned long long d = digest();
            if (!want) want = d;
            if (d != want) return printf("loop mode %d: another result\n", mode), 1;
        }

    // the global bundle adjustment: two thirds of the key frames adjusted, a third of the points optimised themselves
    g_seed = 1618;
    for (size_t i = 0; i < g_pts.size(); i++) {
        *g_pts[i] = g_saved[i];
        if (i % 3 == 0) g_pts[i]->mnBAGlobalForKF = LOOP_KF;
        g_saved[i] = *g_pts[i];
    }
    for (int k = 0; k < NKF; k++) {
        g_kfs[k]->SetPose(g_Tcw[k]);
        const Pose adjusted = nudged(g_poses[k], 1.0);
        if (k % 3 == 0) continue;
        g_kfs[k]->mTcwBefGBA = g_kfs[k]->GetPose();
        g_kfs[k]->SetPose(as_se3(adjusted));
        g_kfs[k]->mnBAGlobalForKF = LOOP_KF;
    }
    std::vector<MapPoint *> gbaPoints;
    for (size_t i = 0; i < g_pts.size(); i++)
        if (g_pts[i]->mnBAGlobalForKF == LOOP_KF || (g_pts[i]->mpRefKF && g_pts[i]->mpRefKF->mnBAGlobalForKF == LOOP_KF)) gbaPoints.push_back(g_pts[i]);
    want = 0;
    for (int r = -2; r < reps; r++)
        for (int mode = 0; mode < 2; mode++) {
            for (size_t i = 0; i < g_pts.size(); i++) *g_pts[i] = g_saved[i];
            LS.Put(g_pts);
            LocalMapSearch::CorrectTimes().device = 0;
            const Clock::time_point t0 = Clock::now();
            if (mode == 0) {
                refcorrect::global_ba(g_pts, LOOP_KF);
                LS.Put(gbaPoints);
            } else {
                LS.ApplyGlobalBA(g_pts, LOOP_KF);
            }
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[3 + mode].push_back(us);
            if (r >= 0 && mode == 1) t[5].push_back(LocalMapSearch::CorrectTimes().device);
            const unsigned long long d = digest();
            if (!want) want = d;
            if (d != want) return printf("gba mode %d: another result\n", mode), 1;
        }

    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    if (LocalMapSearch::CorrectCounts().host != 0) return printf("points went the host way: the measurement is not of the device call\n"), 1;
    const char *names[6] = {"loop_a_host_put", "loop_b_correct", "loop_b_entry", "gba_a_host_put", "gba_b_apply", "gba_b_entry"};
    for (int m = 0; m < 6; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape key_frames %d corrected %d loop_points %d loop_observations %ld map_points %d gba_points %d\n", NKF, K, (int)loopPoints.size(), nobs,
           (int)g_pts.size(), (int)gbaPoints.size());
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
