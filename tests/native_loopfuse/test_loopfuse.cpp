// test_loopfuse.cpp -- ORB_SLAM2::LocalMapSearch::SearchLoopPoints and ::SearchAndFuse on mock KeyFrame / MapPoint objects: a
// current key frame and six covisibles with fresh points, two key frames of the other side of the loop that hold older points of
// the same landmarks (some landmarks twice, as two points), free features, decoy features that a recomputed descriptor prefers, bad
// points.  Every corrected pose is a similarity of scale 0.5, 1.37 or 2 times the key frame's own pose.  The map is built three
// times from one seed: the class works on the first, the reference on the second, the class with the second search of changed
// survivors switched off on the third.  Lists, matches, rows, observations, bad flags and descriptors are compared:
//   -DLOOPFUSE_MOCK  the class runs on the host model of the entry points (mock_loopfuse.cc), the reference is the restatement of the
//                    loops on the objects themselves (ref_loop.h); no device, no liborbhip
//   otherwise        the class runs on liborbhip, the reference is the host union with ORBmatcher::SearchByProjection(pKF, Scw, ...)
//                    and ORBmatcher::Fuse(pKF, Scw, ...) per key frame with the Replace loop (the path before these entry points)
// Prints "ok <loop points> <matches> <replaced> <digest>" and returns 0, or the failed checks.  The digest is over every result and
// the final map, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "ref_loop.h"
#ifndef LOOPFUSE_MOCK
#include "ORBmatcher.h"
#else
extern "C" unsigned long long mock_state_digest();
#endif

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 16) / 65536.f; }

static const int W = 376, H = 241, NLEVELS = 8, NLM = 420, NKF = 9;
static const float S = 1.2f, FX = 300.f, CX = 188.f, CY = 120.5f;
static const float SCALES[3] = {0.5f, 1.37f, 2.0f};

struct World {
    std::vector<KeyFrame *> kfs;                 // 0: the current key frame; 1, 2: the loop side; 3 .. NKF - 1: covisibles of 0
    std::vector<MapPoint *> pts;
    ~World()
    {
        for (size_t i = 0; i < pts.size(); i++) delete pts[i];
        for (size_t i = 0; i < kfs.size(); i++) delete kfs[i];
    }
};

static void flip(uint8_t *d, int bits)
{
    for (int b = 0; b < bits; b++) d[rnd(32)] ^= (uint8_t)(1u << rnd(8));
}

static MapPoint *new_point(World &Wd, const float P[3], const uint8_t *desc)
{
    MapPoint *p = new MapPoint();
    p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
    const float len = sqrtf(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
    for (int k = 0; k < 3; k++) p->mWorldPos.at<float>(k, 0) = P[k], p->mNormalVector.at<float>(k, 0) = P[k] / len;
    memcpy(p->mDescriptor.ptr(0), desc, 32);
    p->mfMaxDistance = 12.f, p->mfMinDistance = 12.f / powf(S, NLEVELS - 1);
    Wd.pts.push_back(p);
    return p;
}

static void hold(KeyFrame *kf, int idx, MapPoint *p)
{
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
}

static void build(World &Wd)
{
    g_seed = 4713;
    struct Landmark { float P[3], angle; uint8_t desc[32]; };
    std::vector<Landmark> L(NLM);
    for (int j = 0; j < NLM; j++) {
        L[j].P[0] = frand(-4, 4), L[j].P[1] = frand(-2.5f, 2.5f), L[j].P[2] = frand(3, 12), L[j].angle = frand(0, 350);
        for (int b = 0; b < 32; b++) L[j].desc[b] = (uint8_t)rnd(256);
    }
    std::vector<std::vector<int> > featOf(NKF, std::vector<int>(NLM, -1));   // feature of landmark j in key frame k
    std::vector<std::vector<uint8_t> > rows(NKF);
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        Wd.kfs.push_back(kf);
        const float a = 0.01f * k, c = cosf(a), s = sinf(a);
        const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, C[3] = {0.12f * k - 0.5f, 0.03f * (k % 3), 0.05f * k};
        kf->Tcw = cv::Mat::zeros(4, 4, CV_32F), kf->Ow = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) {
            double tr = 0;
            for (int q = 0; q < 3; q++) kf->Tcw.at<float>(r, q) = R[3 * r + q], tr -= (double)R[3 * r + q] * (double)C[q];
            kf->Tcw.at<float>(r, 3) = (float)tr;
            kf->Ow.at<float>(r, 0) = C[r];
        }
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
        for (int j = 0; j < NLM + 60; j++) {
            cv::KeyPoint kp;
            uint8_t d[32];
            if (j < NLM) {
                float pc[3];
                for (int r = 0; r < 3; r++)
                    pc[r] = kf->Tcw.at<float>(r, 0) * L[j].P[0] + kf->Tcw.at<float>(r, 1) * L[j].P[1] + kf->Tcw.at<float>(r, 2) * L[j].P[2] + kf->Tcw.at<float>(r, 3);
                if (pc[2] < 0.5f) continue;
                const float u = FX * pc[0] / pc[2] + CX + frand(-0.5f, 0.5f), v = FX * pc[1] / pc[2] + CY + frand(-0.5f, 0.5f);
                if (u < 2 || u > W - 3 || v < 2 || v > H - 3) continue;
                int oct = (int)floorf(logf(12.f / pc[2]) / logf(S));
                oct = oct < 0 ? 0 : oct > NLEVELS - 1 ? NLEVELS - 1 : oct;
                kp = cv::KeyPoint(u, v, 31.f * powf(S, (float)oct), L[j].angle, 50.f, oct, -1);
                memcpy(d, L[j].desc, 32);
                flip(d, 6);
                featOf[k][j] = (int)kf->mvKeys.size();
            } else {
                kp = cv::KeyPoint(frand(2, W - 3), frand(2, H - 3), 31.f, frand(0, 360), 20.f, (int)rnd(NLEVELS), -1);
                for (int b = 0; b < 32; b++) d[b] = (uint8_t)rnd(256);
            }
            kf->mvKeys.push_back(kp);
            rows[k].insert(rows[k].end(), d, d + 32);
        }
    }
    // decoys: beside the feature of every fourth landmark in the later covisibles, a feature that the current key frame's own
    // descriptor of that landmark prefers to the real one (a loop point that survives a Replace in key frame 0 may take it over)
    for (int j = 0; j < NLM; j += 4) {
        if (featOf[0][j] < 0) continue;
        for (int k = 4; k < NKF; k++) {
            if (featOf[k][j] < 0) continue;
            KeyFrame *kf = Wd.kfs[k];
            cv::KeyPoint kp = kf->mvKeys[featOf[k][j]];
            kp.pt.x += 0.7f;
            uint8_t d[32];
            memcpy(d, &rows[0][(size_t)featOf[0][j] * 32], 32);
            flip(d, 2);
            kf->mvKeys.push_back(kp);
            rows[k].insert(rows[k].end(), d, d + 32);
        }
    }
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = Wd.kfs[k];
        kf->mvKeysUn = kf->mvKeys;
        kf->N = (int)kf->mvKeys.size();
        kf->mDescriptors = cv::Mat(kf->N, 32, CV_8U);
        memcpy(kf->mDescriptors.ptr(0), rows[k].data(), rows[k].size());
        kf->mvpMapPoints.assign(kf->N, (MapPoint *)NULL);
    }
    // the loop side: older points in key frames 1 and 2; every seventh landmark as TWO points, one in each (the list holds both)
    std::vector<MapPoint *> oldOf(NLM, (MapPoint *)NULL);
    for (int j = 0; j < NLM; j++) {
        for (int k = 1; k <= 2; k++) {
            if (featOf[k][j] < 0) continue;
            if (j % 7 == 3) {
                hold(Wd.kfs[k], featOf[k][j], new_point(Wd, L[j].P, &rows[k][(size_t)featOf[k][j] * 32]));
                continue;
            }
            if (oldOf[j] ? rnd(2) == 0 : rnd(4) != 0) {
                if (!oldOf[j]) oldOf[j] = new_point(Wd, L[j].P, &rows[k][(size_t)featOf[k][j] * 32]);
                hold(Wd.kfs[k], featOf[k][j], oldOf[j]);
            }
        }
    }
    // this side: fresh points in the current key frame, most of them seen from one or two covisibles as well; some features free
    for (int j = 0; j < NLM; j++) {
        if (featOf[0][j] < 0 || j % 7 == 3) continue;
        if (rnd(100) < 70 || j % 4 == 0) {
            MapPoint *p = new_point(Wd, L[j].P, &rows[0][(size_t)featOf[0][j] * 32]);
            hold(Wd.kfs[0], featOf[0][j], p);
            for (int t = 0; t < 2; t++) {
                const int k = 3 + (int)rnd(NKF - 3);
                if (featOf[k][j] >= 0 && !Wd.kfs[k]->mvpMapPoints[featOf[k][j]] && !p->IsInKeyFrame(Wd.kfs[k])) hold(Wd.kfs[k], featOf[k][j], p);
            }
        }
    }
    // points of the covisibles alone
    for (int j = 1; j < NLM; j += 3) {
        const int k = 3 + (int)rnd(NKF - 3);
        if (featOf[k][j] >= 0 && !Wd.kfs[k]->mvpMapPoints[featOf[k][j]]) hold(Wd.kfs[k], featOf[k][j], new_point(Wd, L[j].P, &rows[k][(size_t)featOf[k][j] * 32]));
    }
    for (size_t i = 0; i < Wd.pts.size(); i += 37) Wd.pts[i]->SetBadFlag();   // bad points that their key frames still hold
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

static int index_of(const World &Wd, MapPoint *p)
{
    if (!p) return -1;
    for (size_t i = 0; i < Wd.pts.size(); i++)
        if (Wd.pts[i] == p) return (int)i;
    return -2;
}
static int index_of(const World &Wd, KeyFrame *kf)
{
    for (size_t i = 0; i < Wd.kfs.size(); i++)
        if (Wd.kfs[i] == kf) return (int)i;
    return -2;
}
static std::vector<int> indices(const World &Wd, const std::vector<MapPoint *> &v)
{
    std::vector<int> out;
    for (size_t i = 0; i < v.size(); i++) out.push_back(index_of(Wd, v[i]));
    return out;
}

// rows, observations, bad flags and descriptors of the two maps, by position
static bool same_maps(World &A, World &B, bool digest)
{
    bool same = A.pts.size() == B.pts.size() && A.kfs.size() == B.kfs.size();
    for (size_t k = 0; k < A.kfs.size() && same; k++) {
        same = A.kfs[k]->mvpMapPoints.size() == B.kfs[k]->mvpMapPoints.size();
        for (size_t i = 0; i < A.kfs[k]->mvpMapPoints.size() && same; i++) {
            const int a = index_of(A, A.kfs[k]->mvpMapPoints[i]), b = index_of(B, B.kfs[k]->mvpMapPoints[i]);
            if (a != b) same = false;
            if (digest) mix((unsigned long long)(a + 2));
        }
    }
    for (size_t i = 0; i < A.pts.size() && same; i++) {
        MapPoint *a = A.pts[i], *b = B.pts[i];
        same = same && a->isBad() == b->isBad() && a->Observations() == b->Observations();
        std::set<std::pair<int, size_t> > oa, ob;
        for (std::map<KeyFrame *, size_t>::iterator it = a->mObservations.begin(); it != a->mObservations.end(); ++it)
            oa.insert(std::make_pair(index_of(A, it->first), it->second));
        for (std::map<KeyFrame *, size_t>::iterator it = b->mObservations.begin(); it != b->mObservations.end(); ++it)
            ob.insert(std::make_pair(index_of(B, it->first), it->second));
        same = same && oa == ob && memcmp(a->mDescriptor.ptr(0), b->mDescriptor.ptr(0), 32) == 0;
        if (!digest) continue;
        mix((unsigned long long)(a->isBad() ? 1 : 0) | ((unsigned long long)a->Observations() << 1));
        for (std::set<std::pair<int, size_t> >::iterator it = oa.begin(); it != oa.end(); ++it) mix(((unsigned long long)it->first << 32) | it->second);
        for (int w = 0; w < 4; w++) {
            unsigned long long v;
            memcpy(&v, a->mDescriptor.ptr(0) + 8 * w, 8);
            mix(v);
        }
    }
    return same;
}

static cv::Mat similarity(KeyFrame *kf, float s)
{
    cv::Mat Scw = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) Scw.at<float>(r, c) = (float)((double)s * (double)kf->Tcw.at<float>(r, c));
    Scw.at<float>(3, 3) = 1.f;
    return Scw;
}

struct Inputs {
    std::vector<KeyFrame *> loopKFs;
    std::vector<std::pair<KeyFrame *, cv::Mat> > corrected;
    std::vector<MapPoint *> matched;
    cv::Mat Scw;
};

static Inputs inputs_of(World &Wd)
{
    Inputs in;
    in.loopKFs.push_back(Wd.kfs[2]), in.loopKFs.push_back(Wd.kfs[1]);          // the covisibles, then the matched key frame
    in.Scw = similarity(Wd.kfs[0], 1.37f);
    int t = 0;
    for (int k = 0; k < NKF; k++)                                              // ascending mnId (docs/parity.md)
        if (k == 0 || k >= 3) in.corrected.push_back(std::make_pair(Wd.kfs[k], similarity(Wd.kfs[k], SCALES[t++ % 3])));
    // what SearchBySim3 left: every ninth feature of the current key frame that holds a point is matched with a loop point
    in.matched.assign(Wd.kfs[0]->N, (MapPoint *)NULL);
    const std::vector<MapPoint *> loop = refloop::LoopPoints(in.loopKFs);
    for (int i = 0, m = 0; i < Wd.kfs[0]->N && m < (int)loop.size(); i += 9, m += 5) in.matched[i] = loop[m];
    return in;
}

int main()
{
    MapPoint::RecomputeOnReplace() = true;               // Replace ends in ComputeDistinctiveDescriptors, as in the reference
    World A, B, C;
    build(A);
    build(B);
    build(C);
    CHECK(same_maps(A, B, false));
    Inputs ia = inputs_of(A), ib = inputs_of(B), ic = inputs_of(C);
    refloop::Stats stats;
    std::vector<MapPoint *> listA, listB, listC;
    int nmA = 0, nmB = 0;
    {
        LocalMapSearch LS(4096);
        LS.InitKeyFrames(16, 1024);
        LS.Put(A.pts);
        for (int k = 0; k < NKF; k++)
            if (k != 7) LS.PutKeyFrame(A.kfs[k]);        // (the last but one is put by the call that needs its row)
        nmA = LS.SearchLoopPoints(A.kfs[0], ia.Scw, ia.loopKFs, listA, ia.matched, 10);
#ifdef LOOPFUSE_MOCK
        listB = refloop::LoopPoints(ib.loopKFs);
        nmB = refloop::SearchByProjection(B.kfs[0], ib.Scw, listB, ib.matched, 10);
#else
        ORBmatcher matcher(0.75f, true);                 // ref: src/LoopClosing.cc:246
        listB = refloop::LoopPoints(ib.loopKFs);
        nmB = matcher.SearchByProjection(B.kfs[0], ib.Scw, listB, ib.matched, 10);
#endif
        CHECK(nmA == nmB && indices(A, listA) == indices(B, listB) && indices(A, ia.matched) == indices(B, ib.matched));
        CHECK(listA.size() >= 200 && nmA >= 20);
        mix((unsigned long long)nmA);
        for (size_t i = 0; i < listA.size(); i++) mix((unsigned long long)(index_of(A, listA[i]) + 2));
        for (size_t i = 0; i < ia.matched.size(); i++) mix((unsigned long long)(index_of(A, ia.matched[i]) + 2));
        printf("# loop points %d, matches %d\n", (int)listA.size(), nmA);

        LS.SearchAndFuse(ia.corrected, listA, 4);
#ifdef LOOPFUSE_MOCK
        refloop::SearchAndFuse(ib.corrected, listB, 4, &stats);
#else
        ORBmatcher fuser(0.8f);                          // ref: src/LoopClosing.cc:649
        for (size_t k = 0; k < ib.corrected.size(); k++) {
            std::vector<MapPoint *> vpReplacePoints(listB.size(), static_cast<MapPoint *>(NULL));
            fuser.Fuse(ib.corrected[k].first, ib.corrected[k].second, listB, 4, vpReplacePoints);
            for (size_t i = 0; i < listB.size(); i++)
                if (vpReplacePoints[i]) vpReplacePoints[i]->Replace(listB[i]);
        }
#endif
        CHECK(same_maps(A, B, true));
        // store and table equal a fresh Put / PutKeyFrame of every object
#ifdef LOOPFUSE_MOCK
        const unsigned long long after = mock_state_digest();
        LS.Clear();
        LS.ClearKeyFrames();
        LS.Put(A.pts);
        for (int k = 0; k < NKF; k++) LS.PutKeyFrame(A.kfs[k]);
        CHECK(after == mock_state_digest());
#else
        LocalMapSearch fresh(4096);
        fresh.InitKeyFrames(16, 1024);
        fresh.Put(A.pts);
        for (int k = 0; k < NKF; k++) fresh.PutKeyFrame(A.kfs[k]);
        for (int cur = 0; cur < NKF; cur++) {            // every row, every flag, every descriptor and position is read by one of these
            std::vector<KeyFrame *> others;
            for (int k = 0; k < NKF; k++)
                if (k != cur) others.push_back(A.kfs[k]);
            std::vector<MapPoint *> l1, l2, m1(A.kfs[cur]->N, (MapPoint *)NULL), m2(A.kfs[cur]->N, (MapPoint *)NULL);
            const cv::Mat Scw = similarity(A.kfs[cur], 2.0f);
            const int n1 = LS.SearchLoopPoints(A.kfs[cur], Scw, others, l1, m1, 10), n2 = fresh.SearchLoopPoints(A.kfs[cur], Scw, others, l2, m2, 10);
            CHECK(n1 == n2 && l1 == l2 && m1 == m2 && !l1.empty());
        }
#endif
    }
    {   // without the second search of survivors whose descriptor changed, the map comes out differently
        LocalMapSearch::ResearchChangedSurvivors() = false;
        LocalMapSearch LS(4096);
        LS.InitKeyFrames(16, 1024);
        LS.Put(C.pts);
        for (int k = 0; k < NKF; k++) LS.PutKeyFrame(C.kfs[k]);
        LS.SearchLoopPoints(C.kfs[0], ic.Scw, ic.loopKFs, listC, ic.matched, 10);
        CHECK(indices(C, listC) == indices(B, listB));
        LS.SearchAndFuse(ic.corrected, listC, 4);
        CHECK(!same_maps(C, B, false));
        LocalMapSearch::ResearchChangedSurvivors() = true;
    }
#ifdef LOOPFUSE_MOCK
    // the scene holds what the sequencing rules are for
    printf("# added %ld replaced %ld; changed and active later %ld, of them with another best feature %ld; held later %ld; added then held %ld\n",
           stats.added, stats.replaced, stats.changedActive, stats.changedDiffers, stats.heldLater, stats.addedThenHeld);
    CHECK(stats.changedActive >= 10 && stats.changedDiffers >= 1 && stats.heldLater >= 10 && stats.addedThenHeld >= 1);
    CHECK(stats.replaced >= 50 && stats.added >= 50);
#endif
    int bad = 0;
    for (size_t i = 0; i < A.pts.size(); i++) bad += A.pts[i]->isBad() ? 1 : 0;
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %d %d %016llx\n", (int)listA.size(), nmA, bad, g_digest);
    return 0;
}
