// test_correct.cpp -- ORB_SLAM2::LocalMapSearch::CorrectLoopPoints and ApplyGlobalBA on mock KeyFrame / MapPoint objects: 30 key frames
// with poses, 1200 points seen from 2 to 6 of them.  The map is built twice from one seed: the class works on one copy, the
// reference's loops written out in ref_correct.h on the other.  CorrectLoopPoints runs over K = 12 key frames in ascending mnId --
// points shared by several of them, a point already stamped with the current key frame's id, points that were never Put, a point
// whose mpRefKF is no observer, one without mpRefKF, a bad point and a point without observations among them -- and ApplyGlobalBA
// over the whole map with a third of the key frames not adjusted.  After each, positions, normals, distance ranges, stamps and poses
// are compared bit for bit between the two maps, and the objects with the resident store (orbhip_map_get).
//   -DCORRECT_MOCK  the class runs on the host model of the entry points (mock_correct.cc); no device, no liborbhip
//   otherwise       the class runs on liborbhip
// Prints "ok <points CorrectLoopPoints moved> <points ApplyGlobalBA moved> <the device way> <the host way> <digest>" and returns 0, or
// the failed checks.  The digest is over every compared value, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "correct_poses.h"
#include "ref_correct.h"

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static const int NKF = 30, NPT = 1200, NFEAT = 320, NLEVELS = 8, K = 12, FIRST = 9;
static const unsigned long CURRENT_ID = 4242, LOOP_KF = 77;
// the special points; each is seen from key frame FIRST + 2, so the loop reaches it
static const int STAMPED = 5, NEVER_PUT[3] = {9, 10, 11}, REF_NO_OBSERVER = 13, NO_REF = 14, BAD = 17, NO_OBSERVATIONS = 21;

struct Probe : LocalMapSearch {   // the store behind the class, for the read-back
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

struct World {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> pts;
    std::vector<Pose> poses;
    std::vector<int> nextFree;   // the next feature of each key frame that holds no point
    ~World()
    {
        for (size_t i = 0; i < pts.size(); i++) delete pts[i];
        for (size_t i = 0; i < kfs.size(); i++) delete kfs[i];
    }
};

static void observe(World &W, MapPoint *p, int k)
{
    KeyFrame *kf = W.kfs[k];
    if (p->IsInKeyFrame(kf) || W.nextFree[k] >= kf->N) return;
    const int idx = W.nextFree[k]++;
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
    if (!p->mpRefKF) p->mpRefKF = kf;
}

static void build(World &W)
{
    g_seed = 31337;
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        W.kfs.push_back(kf);
        W.poses.push_back(random_pose());
        kf->N = NFEAT;
        kf->SetPose(as_se3(W.poses[k]));
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = 1.2f, kf->mfLogScaleFactor = logf(1.2f);
        float s = 1.f;
        for (int l = 0; l < NLEVELS; l++, s *= 1.2f) {
            kf->mvScaleFactors.push_back(s);
            kf->mvLevelSigma2.push_back(s * s);
            kf->mvInvLevelSigma2.push_back(1.f / (s * s));
        }
        kf->mDescriptors = cv::Mat(NFEAT, 32, CV_8U);
        for (int i = 0; i < NFEAT; i++) {
            kf->mvKeys.push_back(cv::KeyPoint((float)drand(2, 637), (float)drand(2, 477), 31.f, (float)drand(0, 360), 20.f, (int)rnd(NLEVELS), -1));
            for (int b = 0; b < 32; b++) kf->mDescriptors.ptr(i)[b] = (uint8_t)rnd(256);
        }
        kf->mvKeysUn = kf->mvKeys;
        kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
        W.nextFree.push_back(0);
    }
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new MapPoint();
        W.pts.push_back(p);
        p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c, 0) = (float)drand(-6, 6) + (c == 2 ? 9.f : 0.f), p->mNormalVector.at<float>(c, 0) = 0.f;
        for (int b = 0; b < 32; b++) p->mDescriptor.ptr(0)[b] = (uint8_t)rnd(256);
        p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
        if (j < 30) observe(W, p, FIRST + 2);
        const int n = 2 + (int)rnd(5);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 400; tries++) observe(W, p, (int)rnd(NKF));
    }
    // the special points
    W.pts[STAMPED]->mnCorrectedByKF = CURRENT_ID;
    for (int k = 0; k < NKF; k++)
        if (!W.pts[REF_NO_OBSERVER]->IsInKeyFrame(W.kfs[k])) { W.pts[REF_NO_OBSERVER]->mpRefKF = W.kfs[k]; break; }
    W.pts[NO_REF]->mpRefKF = NULL;
    W.pts[BAD]->SetBadFlag();
    W.pts[NO_OBSERVATIONS]->mObservations.clear();
    W.pts[NO_OBSERVATIONS]->nObs = 0;
}

// the K corrections, key frames FIRST .. FIRST + K - 1 in ascending mnId; the same values for both maps
static std::vector<LoopCorrection> corrections(World &W)
{
    g_seed = 2718;
    std::vector<LoopCorrection> v;
    for (int j = 0; j < K; j++) {
        const Pose corrected = nudged(W.poses[FIRST + j], drand(0.9, 1.1));
        LoopCorrection L;
        L.pKF = W.kfs[FIRST + j];
        L.Siw = as_sim3(W.poses[FIRST + j]);
        L.correctedSwi = inverse(corrected);
        L.correctedTiw = as_se3(corrected);
        v.push_back(L);
    }
    return v;
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static bool same3(const cv::Mat &a, const cv::Mat &b)
{
    bool ok = true;
    for (int c = 0; c < 3; c++) ok = ok && bits(a.at<float>(c, 0)) == bits(b.at<float>(c, 0)), mix(bits(a.at<float>(c, 0)));
    return ok;
}

// points, stamps and poses of the two maps, and the store behind the class, bit for bit
static void compare(Probe &LS, World &A, World &B, const std::vector<MapPoint *> &inStore)
{
    bool pos = true, geo = true, stamps = true, poses = true, store = true;
    for (size_t i = 0; i < A.pts.size(); i++) {
        MapPoint *a = A.pts[i], *b = B.pts[i];
        pos = pos && same3(a->mWorldPos, b->mWorldPos);
        geo = geo && same3(a->mNormalVector, b->mNormalVector) && bits(a->mfMinDistance) == bits(b->mfMinDistance) &&
              bits(a->mfMaxDistance) == bits(b->mfMaxDistance);
        mix(((unsigned long long)bits(a->mfMinDistance) << 32) | bits(a->mfMaxDistance));
        stamps = stamps && a->mnCorrectedByKF == b->mnCorrectedByKF;
        if (a->mnCorrectedByKF == CURRENT_ID && (int)i != STAMPED)   // (the two maps' key frames have their own mnId ranges)
            stamps = stamps && a->mnCorrectedReference - A.kfs[0]->mnId == b->mnCorrectedReference - B.kfs[0]->mnId;
        mix(a->mnCorrectedByKF);
    }
    for (size_t k = 0; k < A.kfs.size(); k++) {
        poses = poses && same3(A.kfs[k]->Ow, B.kfs[k]->Ow);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses = poses && bits(A.kfs[k]->Tcw.at<float>(r, c)) == bits(B.kfs[k]->Tcw.at<float>(r, c));
    }
    CHECK(pos);
    CHECK(geo);
    CHECK(stamps);
    CHECK(poses);
    const size_t n = inStore.size();
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) keys[i] = (uint64_t)inStore[i]->mnId + 1;
    std::vector<float> p(3 * n), nrm(3 * n), mn(n), mx(n);
    std::vector<uint8_t> d(32 * n);
    CHECK(orbhip_map_get(LS.ctx(), (int)n, keys.data(), p.data(), nrm.data(), mn.data(), mx.data(), d.data(), NULL) == ORBHIP_OK);
    for (size_t i = 0; i < n; i++) {
        MapPoint *a = inStore[i];
        store = store && memcmp(a->mDescriptor.ptr(0), &d[32 * i], 32) == 0 && bits(a->mfMinDistance) == bits(mn[i]) && bits(a->mfMaxDistance) == bits(mx[i]);
        for (int c = 0; c < 3; c++)
            store = store && bits(a->mWorldPos.at<float>(c, 0)) == bits(p[3 * i + c]) && bits(a->mNormalVector.at<float>(c, 0)) == bits(nrm[3 * i + c]);
    }
    CHECK(store);
}

int main()
{
    World A, B;
    build(A);
    build(B);
    Probe LS(4096);
    std::vector<MapPoint *> put, inStore;
    for (int j = 0; j < NPT; j++)
        if (j != NEVER_PUT[0] && j != NEVER_PUT[1] && j != NEVER_PUT[2]) put.push_back(A.pts[j]);
    LS.Put(put);

    // ---- CorrectLoop ----
    const std::vector<LoopCorrection> ca = corrections(A), cb = corrections(B);
    int shared = 0;   // points that several corrected key frames hold: the first owns them
    for (int j = 0; j < NPT; j++) {
        int n = 0;
        for (int k = FIRST; k < FIRST + K; k++) n += A.pts[j]->IsInKeyFrame(A.kfs[k]) ? 1 : 0;
        shared += n >= 2 ? 1 : 0;
    }
    CHECK(shared >= 100);
    const float before = A.pts[STAMPED]->mWorldPos.at<float>(0, 0);
    const int movedB = refcorrect::correct_loop(cb, CURRENT_ID);
    const int movedA = LS.CorrectLoopPoints(ca, CURRENT_ID);
    CHECK(movedA == movedB && movedA >= 600 && movedA < NPT);
    CHECK(bits(A.pts[STAMPED]->mWorldPos.at<float>(0, 0)) == bits(before));   // stamped before: left alone
    CHECK(A.pts[NO_OBSERVATIONS]->mnCorrectedByKF == CURRENT_ID && A.pts[NO_OBSERVATIONS]->mfMaxDistance == 12.f);   // moved, not refreshed
    CHECK(A.pts[BAD]->mnCorrectedByKF == 0);
    const long dev1 = LocalMapSearch::CorrectCounts().device, host1 = LocalMapSearch::CorrectCounts().host;
    printf("# CorrectLoopPoints: %d points, %ld the device way, %ld the host way, %d shared\n", movedA, dev1, host1, shared);
    CHECK(host1 == 5 && dev1 == movedA - 5);          // three never Put, one whose mpRefKF is no observer, one without mpRefKF
    inStore = put;
    for (int i = 0; i < 3; i++) inStore.push_back(A.pts[NEVER_PUT[i]]);   // Put by the host way
    compare(LS, A, B, inStore);

    // ---- the global bundle adjustment's update ----
    World *Ws[2] = {&A, &B};
    for (int w = 0; w < 2; w++) {
        World &W = *Ws[w];
        g_seed = 1618;
        for (int k = 0; k < NKF; k++) {
            const Pose adjusted = nudged(W.poses[k], 1.0);
            if (k % 3 == 0) continue;                 // a third of the key frames: not adjusted
            W.kfs[k]->mTcwBefGBA = W.kfs[k]->GetPose();
            W.kfs[k]->SetPose(as_se3(adjusted));
            W.kfs[k]->mnBAGlobalForKF = LOOP_KF;
        }
        for (int j = 0; j < NPT; j++) {
            MapPoint *p = W.pts[j];
            cv::Mat g(3, 1, CV_32F);
            for (int c = 0; c < 3; c++) g.at<float>(c, 0) = p->mWorldPos.at<float>(c, 0) + (float)drand(-0.1, 0.1);
            p->mPosGBA = g;
            if (j % 3 == 0 || j == NO_REF) p->mnBAGlobalForKF = LOOP_KF;   // optimised by the adjustment: takes mPosGBA
        }
    }
    LS.Erase(A.pts[NEVER_PUT[0]]);                    // not in the store: the host way (one takes mPosGBA, one follows its
    LS.Erase(A.pts[NEVER_PUT[1]]);                    // reference key frame FIRST + 2), and Put again
    CHECK(A.pts[NEVER_PUT[0]]->mnBAGlobalForKF == LOOP_KF && A.pts[NEVER_PUT[1]]->mnBAGlobalForKF != LOOP_KF &&
          A.pts[NEVER_PUT[1]]->mpRefKF == A.kfs[FIRST + 2] && A.kfs[FIRST + 2]->mnBAGlobalForKF == LOOP_KF);
    const int gbaB = refcorrect::global_ba(B.pts, LOOP_KF);
    const int gbaA = LS.ApplyGlobalBA(A.pts, LOOP_KF);
    CHECK(gbaA == gbaB && gbaA >= 800 && gbaA < NPT - 50);   // points of the key frames that were not adjusted stay
    const long dev2 = LocalMapSearch::CorrectCounts().device - dev1, host2 = LocalMapSearch::CorrectCounts().host - host1;
    printf("# ApplyGlobalBA: %d points, %ld the device way, %ld the host way\n", gbaA, dev2, host2);
    CHECK(host2 == 2 && dev2 + host2 == gbaA);
    compare(LS, A, B, inStore);

    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %d %ld %ld %016llx\n", movedA, gbaA, dev1 + dev2, host1 + host2, g_digest);
    return 0;
}
