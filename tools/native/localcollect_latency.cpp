// localcollect_latency.cpp -- Tracking::UpdateLocalMap + SearchLocalPoints per frame from a C++ caller, host loops against
// the device path (tools/localcollect_latency.py runs it).  A synthetic map of K key frames x 1000
// features whose points are shared by about four neighbouring key frames, a 1000-feature 752 x 480 frame that matched 300 of
// them across the whole map, so that all K key frames enter the local map.  Per repetition, alternating in one process:
//   a_host_loops      the host restatement of the reference's two loops (tests/native_localcollect/ref_update_local_map.h)
//   b_host_search     a + LocalMapSearch::SearchLocalPoints (orbhip_search_local_points): the path without this feature
//   c_device_track    LocalMapSearch::UpdateLocalKeyFrames (orbhip_map_vote + the graph step) + TrackLocalPoints
//                     (orbhip_track_local_points)
//   d_collect         orbhip_map_collect alone
//   kf_set_one / kf_put_1000   SetMapPoint of one entry / PutKeyFrame of a 1000-entry row
// b and c must leave the same local map, the same matches and the same counts, or the program fails.
// usage: localcollect_latency K reps        prints "<name> median <us> p10 <us> p90 <us>" lines
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_update_local_map.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 2024;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand() { return (float)rnd(1 << 20) / (float)(1 << 20); }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static const int N = 1000, NLEVELS = 8;
static const float FX = 458.f, FY = 457.f, CX = 376.f, CY = 240.f, W = 752.f, H = 480.f;

struct Proj { float u, v; int level; };

static MapPoint *make_point(Proj *pr)
{
    MapPoint *p = new MapPoint();
    const float u = -60.f + frand() * (W + 120.f), v = -40.f + frand() * (H + 80.f), z = 2.f + 6.f * frand();
    const float x = (u - CX) * z / FX, y = (v - CY) * z / FY, d = std::sqrt(x * x + y * y + z * z);
    p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
    p->mWorldPos.at<float>(0, 0) = x, p->mWorldPos.at<float>(1, 0) = y, p->mWorldPos.at<float>(2, 0) = z;
    p->mNormalVector.at<float>(0, 0) = -x / d, p->mNormalVector.at<float>(1, 0) = -y / d, p->mNormalVector.at<float>(2, 0) = -z / d;
    const int level = (int)rnd(NLEVELS);
    p->mfMaxDistance = d * std::pow(1.2f, level - 0.5f), p->mfMinDistance = p->mfMaxDistance / std::pow(1.2f, NLEVELS - 1);
    for (int b = 0; b < 32; b++) p->mDescriptor.ptr(0)[b] = (unsigned char)rnd(256);
    pr->u = u, pr->v = v, pr->level = level;
    return p;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m * 9 / 10]);
}

int main(int argc, char **argv)
{
    if (argc < 3) return fprintf(stderr, "usage: %s key_frames reps\n", argv[0]), 2;
    const int K = atoi(argv[1]), R = atoi(argv[2]), WARM = 10;
    if (K < 1 || K > 4096 || R < 1) return 2;
    Frame::fx = FX, Frame::fy = FY, Frame::cx = CX, Frame::cy = CY;
    Frame::mnMinX = 0, Frame::mnMaxX = W, Frame::mnMinY = 0, Frame::mnMaxY = H;
    Frame::mfGridElementWidthInv = 64.f / W, Frame::mfGridElementHeightInv = 48.f / H;

    const int pool = std::max(K * 250, 1200);
    Probe S(pool + 16);
    S.InitKeyFrames(K + 1, N);
    std::vector<MapPoint *> pts(pool);
    std::vector<Proj> proj(pool);
    for (int i = 0; i < pool; i++) pts[i] = make_point(&proj[i]);
    S.Put(pts);
    // key frame k: 850 points of a 1000-point window that advances by 250 per key frame, at shuffled feature indices
    std::vector<KeyFrame *> kfs(K);
    for (int k = 0; k < K; k++) {
        KeyFrame *kf = kfs[k] = new KeyFrame();
        kf->N = N;
        kf->mvpMapPoints.assign(N, (MapPoint *)NULL);
        std::vector<int> at(N);
        for (int i = 0; i < N; i++) at[i] = i;
        for (int i = N - 1; i > 0; i--) std::swap(at[i], at[rnd(i + 1)]);
        for (int j = 0; j < 850; j++) {
            MapPoint *p = pts[(k * 250 + j) % pool];
            if (p->IsInKeyFrame(kf)) continue;
            kf->AddMapPoint(p, at[j]);
            p->AddObservation(kf, at[j]);
        }
    }
    for (int k = 0; k < K; k++) {
        for (int d = 1; d <= 3; d++) {
            if (k - d >= 0) kfs[k]->mvpOrderedConnectedKeyFrames.push_back(kfs[k - d]);
            if (k + d < K) kfs[k]->mvpOrderedConnectedKeyFrames.push_back(kfs[k + d]);
        }
        if (k > 0) kfs[k]->mpParent = kfs[k - 1], kfs[k - 1]->mspChildrens.insert(kfs[k]);
    }
    for (int i = 0; i < pool; i++) S.UpdateFlags(pts[i]);
    for (int k = 0; k < K; k++) S.PutKeyFrame(kfs[k]);

    // the frame: half of its features lie where a point projects and carry its descriptor; 300 already hold a point
    Frame dummy, F;
    F.N = N;
    F.mvKeys.resize(N), F.mvKeysUn.resize(N);
    F.mDescriptors = cv::Mat(N, 32, CV_8U);
    F.mvpMapPoints.assign(N, (MapPoint *)NULL);
    F.mnScaleLevels = NLEVELS, F.mfScaleFactor = 1.2f, F.mfLogScaleFactor = std::log(1.2f);
    for (int l = 0; l < NLEVELS; l++) F.mvScaleFactors.push_back(std::pow(1.2f, l));
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = r == c ? 1.f : 0.f;
    for (int i = 0; i < N; i++) {
        cv::KeyPoint &kp = F.mvKeysUn[i];
        int src = (int)rnd(pool);
        for (int tries = 0; tries < 50 && !(proj[src].u > 1 && proj[src].u < W - 1 && proj[src].v > 1 && proj[src].v < H - 1); tries++) src = (int)rnd(pool);
        if (i % 2 == 0) {
            kp.pt.x = proj[src].u + frand() - 0.5f, kp.pt.y = proj[src].v + frand() - 0.5f, kp.octave = proj[src].level;
            memcpy(F.mDescriptors.ptr(i), pts[src]->mDescriptor.ptr(0), 32);
        } else {
            kp.pt.x = 1 + frand() * (W - 2), kp.pt.y = 1 + frand() * (H - 2), kp.octave = (int)rnd(NLEVELS);
            for (int b = 0; b < 32; b++) F.mDescriptors.ptr(i)[b] = (unsigned char)rnd(256);
        }
        kp.angle = 0, kp.size = 31, kp.response = 1, kp.class_id = -1;
        if (i % 10 < 3) F.mvpMapPoints[i] = pts[rnd(pool)];
    }
    F.mvKeys = F.mvKeysUn;
    const std::vector<MapPoint *> frameBefore = F.mvpMapPoints;

    std::vector<KeyFrame *> kfsA, kfsC;
    std::vector<MapPoint *> mpsA, mpsC;
    KeyFrame *refA = NULL, *refC = NULL;
    std::vector<double> ta, tb, tc, td, tset, tput;
    std::vector<uint64_t> kfKeys, local(pool);
    std::vector<MapPoint *> afterB;
    int ntmB = 0, ntmC = 0, nmB = 0, nmC = 0, nlocal = 0;
    for (int it = 0; it < R + WARM; it++) {
        for (int side = 0; side < 2; side++) {
            // untimed: the objects as a new frame finds them, then the first loop of SearchLocalPoints (ref: :2318-2334)
            for (int k = 0; k < K; k++) kfs[k]->mnTrackReferenceForFrame = 0;
            for (int i = 0; i < pool; i++) pts[i]->mnTrackReferenceForFrame = 0, pts[i]->mnLastFrameSeen = 0, pts[i]->mbTrackInView = false;
            F.mvpMapPoints = frameBefore;
            for (int i = 0; i < N; i++)
                if (F.mvpMapPoints[i]) F.mvpMapPoints[i]->mnLastFrameSeen = F.mnId;
            if (side == 0) {
                const Clock::time_point t0 = Clock::now();
                refrestate::ref_update(F, kfsA, mpsA, refA);
                const Clock::time_point t1 = Clock::now();
                nmB = S.SearchLocalPoints(F, mpsA, 1.0f, 0.5f, &ntmB);
                const Clock::time_point t2 = Clock::now();
                afterB = F.mvpMapPoints;
                if (it >= WARM) {
                    ta.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
                    tb.push_back(std::chrono::duration<double, std::micro>(t2 - t0).count());
                }
            } else {
                const Clock::time_point t3 = Clock::now();
                S.UpdateLocalKeyFrames(F, kfsC, refC);
                nmC = S.TrackLocalPoints(F, kfsC, mpsC, 1.0f, 0.5f, &ntmC);
                const Clock::time_point t4 = Clock::now();
                if (it >= WARM) tc.push_back(std::chrono::duration<double, std::micro>(t4 - t3).count());
                if (F.mvpMapPoints != afterB) return printf("FAILED: the two paths leave different matches in the frame\n"), 1;
            }
        }
        if (kfsC != kfsA || mpsC != mpsA || refC != refA || ntmC != ntmB || nmC != nmB)
            return printf("FAILED: the two paths differ (%d / %d key frames, %d / %d points, %d / %d in view, %d / %d matches)\n",
                          (int)kfsA.size(), (int)kfsC.size(), (int)mpsA.size(), (int)mpsC.size(), ntmB, ntmC, nmB, nmC), 1;
        kfKeys.resize(kfsC.size());
        for (size_t k = 0; k < kfsC.size(); k++) kfKeys[k] = (uint64_t)kfsC[k]->mnId + 1;
        const Clock::time_point t5 = Clock::now();
        if (orbhip_map_collect(S.ctx(), (int)kfKeys.size(), kfKeys.data(), local.data(), pool, &nlocal) != ORBHIP_OK) return printf("FAILED: collect\n"), 1;
        const Clock::time_point t6 = Clock::now();
        const size_t idx = (size_t)pts[0]->GetIndexInKeyFrame(kfs[0]);
        S.SetMapPoint(kfs[0], idx, pts[0]);
        const Clock::time_point t7 = Clock::now();
        S.PutKeyFrame(kfs[0]);
        const Clock::time_point t8 = Clock::now();
        if (it >= WARM) {
            td.push_back(std::chrono::duration<double, std::micro>(t6 - t5).count());
            tset.push_back(std::chrono::duration<double, std::micro>(t7 - t6).count());
            tput.push_back(std::chrono::duration<double, std::micro>(t8 - t7).count());
        }
    }
    if (OrbHipErrorCount() != 0 || nlocal != (int)mpsA.size()) return printf("FAILED: %lu errors, %d / %d points\n", OrbHipErrorCount(), nlocal, (int)mpsA.size()), 1;
    printf("shape key_frames %d local_key_frames %d local_points %d in_view %d matches %d\n", K, (int)kfsA.size(), (int)mpsA.size(), ntmB, nmB);
    report("a_host_loops", ta);
    report("b_host_search", tb);
    report("c_device_track", tc);
    report("d_collect", td);
    report("kf_set_one", tset);
    report("kf_put_1000", tput);
    return 0;
}
