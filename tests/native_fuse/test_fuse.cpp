// test_fuse.cpp -- ORB_SLAM2::LocalMapSearch::FuseInTargets and ::FuseCandidates on mock KeyFrame / MapPoint objects: a new key
// frame with fresh points, eight neighbours that hold older points of the same landmarks (some seen only once: the fresh point
// survives the Replace and its descriptor is recomputed), free features, decoy features that the fresh point's first descriptor
// prefers, bad points, stereo and monocular key frames.  Three rounds -- the new key frame into its neighbours, a neighbour into
// the others (on the map the first round left resident), and 70 targets in one call -- each with both passes.  The map is built
// twice from one seed: the class works on one copy, the reference on the other, and after every pass return values, rows,
// observations, bad flags and descriptors are compared:
//   -DFUSE_MOCK  the class runs on the host model of the entry points (mock_fuse.cc), the reference is the restatement of
//                SearchInNeighbors' two loops on the objects themselves (ref_fuse.h); no device, no liborbhip
//   otherwise    the class runs on liborbhip, the reference is ORBmatcher::Fuse called per target (the path before these entry points)
// Prints "ok <rounds> <fused in targets> <fused candidates> <replaced> <digest>" and returns 0, or the failed checks.  The digest
// is over every return value and the final map, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "ref_fuse.h"
#ifndef FUSE_MOCK
#include "ORBmatcher.h"
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
static const float S = 1.2f, FX = 300.f, CX = 188.f, CY = 120.5f, MBF = 40.f;

struct World {
    std::vector<KeyFrame *> kfs;                 // kfs[0]: the new key frame; 1 .. NKF - 1: its neighbours
    std::vector<MapPoint *> pts;
    std::vector<std::vector<int> > lm;           // landmark of each feature, -1 = clutter or decoy
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
    g_seed = 4711;
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
        Wd.lm.push_back(std::vector<int>());
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
        kf->fx = kf->fy = FX, kf->cx = CX, kf->cy = CY, kf->mbf = MBF;
        kf->mnMinX = 0, kf->mnMaxX = W, kf->mnMinY = 0, kf->mnMaxY = H;
        kf->mfGridElementWidthInv = (float)FRAME_GRID_COLS / W, kf->mfGridElementHeightInv = (float)FRAME_GRID_ROWS / H;
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = S, kf->mfLogScaleFactor = logf(S);
        for (int l = 0; l < NLEVELS; l++) {
            kf->mvScaleFactors.push_back(powf(S, (float)l));
            kf->mvLevelSigma2.push_back(kf->mvScaleFactors[l] * kf->mvScaleFactors[l]);
            kf->mvInvLevelSigma2.push_back(1.0f / kf->mvLevelSigma2[l]);
        }
        const bool stereo = k % 3 != 1;
        for (int j = 0; j < NLM + 60; j++) {
            cv::KeyPoint kp;
            uint8_t d[32];
            float z = 0;
            if (j < NLM) {
                float pc[3];
                for (int r = 0; r < 3; r++)
                    pc[r] = kf->Tcw.at<float>(r, 0) * L[j].P[0] + kf->Tcw.at<float>(r, 1) * L[j].P[1] + kf->Tcw.at<float>(r, 2) * L[j].P[2] + kf->Tcw.at<float>(r, 3);
                if (pc[2] < 0.5f) continue;
                const float u = FX * pc[0] / pc[2] + CX + frand(-0.5f, 0.5f), v = FX * pc[1] / pc[2] + CY + frand(-0.5f, 0.5f);
                if (u < 2 || u > W - 3 || v < 2 || v > H - 3) continue;
                z = pc[2];
                int oct = (int)floorf(logf(12.f / z) / logf(S));
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
            if (k != 5) kf->mvuRight.push_back(stereo && z > 0 && rnd(10) < 7 ? kp.pt.x - MBF / z + frand(-0.3f, 0.3f) : -1.f);   // (5: no vector at all)
            rows[k].insert(rows[k].end(), d, d + 32);
            Wd.lm[k].push_back(j < NLM ? j : -1);
        }
    }
    // decoys: beside the feature of every fourth landmark in the later neighbours, a feature that the new key frame's own
    // descriptor of that landmark prefers to the real one
    for (int j = 0; j < NLM; j += 4) {
        if (featOf[0][j] < 0) continue;
        for (int k = 3; k < NKF; k++) {
            if (featOf[k][j] < 0) continue;
            KeyFrame *kf = Wd.kfs[k];
            cv::KeyPoint kp = kf->mvKeys[featOf[k][j]];
            kp.pt.x += 0.7f;
            uint8_t d[32];
            memcpy(d, &rows[0][(size_t)featOf[0][j] * 32], 32);
            flip(d, 2);
            kf->mvKeys.push_back(kp);
            if (k != 5) kf->mvuRight.push_back(-1.f);
            rows[k].insert(rows[k].end(), d, d + 32);
            Wd.lm[k].push_back(-1);
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
    // the older points: seen from the neighbours; every fourth from one early neighbour alone
    std::vector<MapPoint *> oldOf(NLM, (MapPoint *)NULL);
    for (int j = 0; j < NLM; j++) {
        for (int k = 1; k < NKF; k++) {
            if (featOf[k][j] < 0) continue;
            const bool sees = j % 4 == 0 ? (oldOf[j] == NULL && k <= 2) : rnd(2) == 0;
            if (!sees) continue;
            if (!oldOf[j]) oldOf[j] = new_point(Wd, L[j].P, &rows[k][(size_t)featOf[k][j] * 32]);
            hold(Wd.kfs[k], featOf[k][j], oldOf[j]);
        }
    }
    // the new key frame: fresh points (also seen from one later neighbour, as CreateNewMapPoints leaves them), older points, nothing
    for (int j = 0; j < NLM; j++) {
        if (featOf[0][j] < 0) continue;
        const unsigned r = rnd(100);
        if (r < 55 || j % 4 == 0) {
            MapPoint *p = new_point(Wd, L[j].P, &rows[0][(size_t)featOf[0][j] * 32]);
            hold(Wd.kfs[0], featOf[0][j], p);
            const int k = 4 + (int)rnd(NKF - 4);
            if (featOf[k][j] >= 0 && !Wd.kfs[k]->mvpMapPoints[featOf[k][j]]) hold(Wd.kfs[k], featOf[k][j], p);
        } else if (r < 70 && oldOf[j])
            hold(Wd.kfs[0], featOf[0][j], oldOf[j]);
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

// rows, observations, bad flags and descriptors of the two maps, by position
static void compare_maps(World &A, World &B)
{
    CHECK(A.pts.size() == B.pts.size() && A.kfs.size() == B.kfs.size());
    for (size_t k = 0; k < A.kfs.size(); k++) {
        CHECK(A.kfs[k]->mvpMapPoints.size() == B.kfs[k]->mvpMapPoints.size());
        bool same = true;
        for (size_t i = 0; i < A.kfs[k]->mvpMapPoints.size(); i++) {
            const int a = index_of(A, A.kfs[k]->mvpMapPoints[i]), b = index_of(B, B.kfs[k]->mvpMapPoints[i]);
            same = same && a == b;
            mix((unsigned long long)(a + 2));
        }
        CHECK(same);
    }
    bool flags = true, obs = true, desc = true;
    for (size_t i = 0; i < A.pts.size(); i++) {
        MapPoint *a = A.pts[i], *b = B.pts[i];
        flags = flags && a->isBad() == b->isBad() && a->Observations() == b->Observations();
        obs = obs && a->mObservations.size() == b->mObservations.size();
        std::set<std::pair<int, size_t> > oa, ob;
        for (std::map<KeyFrame *, size_t>::iterator it = a->mObservations.begin(); it != a->mObservations.end(); ++it)
            oa.insert(std::make_pair(index_of(A, it->first), it->second));
        for (std::map<KeyFrame *, size_t>::iterator it = b->mObservations.begin(); it != b->mObservations.end(); ++it)
            ob.insert(std::make_pair(index_of(B, it->first), it->second));
        obs = obs && oa == ob;
        desc = desc && memcmp(a->mDescriptor.ptr(0), b->mDescriptor.ptr(0), 32) == 0;
        mix((unsigned long long)(a->isBad() ? 1 : 0) | ((unsigned long long)a->Observations() << 1));
        for (std::set<std::pair<int, size_t> >::iterator it = oa.begin(); it != oa.end(); ++it) mix(((unsigned long long)it->first << 32) | it->second);
        for (int w = 0; w < 4; w++) {
            unsigned long long v;
            memcpy(&v, a->mDescriptor.ptr(0) + 8 * w, 8);
            mix(v);
        }
    }
    CHECK(flags);
    CHECK(obs);
    CHECK(desc);
}

static long g_inTargets = 0, g_candidates = 0;
static reffuse::Stats g_stats;

static std::vector<int> ref_targets(KeyFrame *pKF, const std::vector<KeyFrame *> &targets)
{
#ifdef FUSE_MOCK
    return reffuse::FuseInTargets(pKF, targets, 3.0f, &g_stats);
#else
    ORBmatcher matcher;                                  // ref: src/LocalMapping.cc:2548
    const std::vector<MapPoint *> vpMapPointMatches = pKF->GetMapPointMatches();
    std::vector<int> n;
    for (size_t k = 0; k < targets.size(); k++) n.push_back(matcher.Fuse(targets[k], vpMapPointMatches));
    return n;
#endif
}

static int ref_candidates(KeyFrame *pKF, const std::vector<KeyFrame *> &targets)
{
#ifdef FUSE_MOCK
    return reffuse::FuseCandidates(pKF, targets, 3.0f);
#else
    ORBmatcher matcher;
    return matcher.Fuse(pKF, reffuse::Candidates(targets));
#endif
}

static void round_of(LocalMapSearch &LS, World &A, World &B, int cur, const std::vector<int> &targets)
{
    std::vector<KeyFrame *> ta, tb;
    for (size_t k = 0; k < targets.size(); k++) ta.push_back(A.kfs[targets[k]]), tb.push_back(B.kfs[targets[k]]);
    const std::vector<int> na = LS.FuseInTargets(A.kfs[cur], ta), nb = ref_targets(B.kfs[cur], tb);
    CHECK(na == nb);
    for (size_t k = 0; k < na.size(); k++) mix((unsigned long long)na[k]), g_inTargets += na[k];
    compare_maps(A, B);
    const int ca = LS.FuseCandidates(A.kfs[cur], ta), cb = ref_candidates(B.kfs[cur], tb);
    CHECK(ca == cb);
    mix((unsigned long long)ca), g_candidates += ca;
    compare_maps(A, B);
}

int main()
{
    MapPoint::RecomputeOnReplace() = true;               // Replace ends in ComputeDistinctiveDescriptors, as in the reference
    World A, B;
    build(A);
    build(B);
    LocalMapSearch LS(4096);
    LS.InitKeyFrames(16, 1024);
    LS.Put(A.pts);
    for (int k = 0; k < NKF; k++)
        if (k != 7) LS.PutKeyFrame(A.kfs[k]);            // (the last but one is put by the pass that needs its row)
    compare_maps(A, B);

    std::vector<int> t1, t2, t3;
    for (int k = 1; k < NKF; k++) t1.push_back(k);
    round_of(LS, A, B, 0, t1);                            // the new key frame into its neighbours
    const long first = g_inTargets, firstCand = g_candidates;
    printf("# first round: %ld fused in the targets, %ld candidates fused\n", first, firstCand);
    CHECK(first >= 400 && firstCand >= 50);
    const int o2[] = {1, 2, 4, 5, 0, 6};
    t2.assign(o2, o2 + 6);
    round_of(LS, A, B, 3, t2);                            // a neighbour into the others, on the resident map as the first round left it
    for (int k = 0; k < 70; k++) t3.push_back(k % 8 < 6 ? k % 8 : k % 8 + 1);   // 70 targets: two device calls, keys repeat
    round_of(LS, A, B, 6, t3);
#ifdef FUSE_MOCK
    // the scene holds what the rule about changed descriptors is for: points that survived a Replace in an early target, are
    // active in a later one and find another feature there with their new descriptor than with their old
    printf("# added %ld replaced %ld; changed and active later %ld, of them with another best feature %ld\n", g_stats.added,
           g_stats.replaced, g_stats.changedActive, g_stats.changedDiffers);
    CHECK(g_stats.changedActive >= 10 && g_stats.changedDiffers >= 1);
    CHECK(g_stats.replaced >= 50 && g_stats.added >= 50);
#endif
    int bad = 0;
    for (size_t i = 0; i < A.pts.size(); i++) bad += A.pts[i]->isBad() ? 1 : 0;
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok 3 %ld %ld %d %016llx\n", g_inTargets, g_candidates, bad, g_digest);
    return 0;
}
