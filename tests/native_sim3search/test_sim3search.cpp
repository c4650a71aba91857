// test_sim3search.cpp -- ORB_SLAM2::LocalMapSearch::SearchBySim3 on mock KeyFrame / MapPoint objects: the two sides of a loop, two key
// frames that see the same 300 landmarks through a similarity of scale 1.37, each holding its own points for most of them (so most
// landmarks are two points, one per map), free features, features without a landmark, bad points and some entries of vpMatches12
// filled beforehand as SearchByBoW leaves them.  The map is built three times from one seed: the class works on the first, the
// reference on the second, the host restatement counts what the scene holds on the third.
//   -DSIM3SEARCH_MOCK  the class runs on the host model of the entry point (mock_sim3search.cc), the reference is the restatement of
//                      the loops on the objects themselves (ref_sim3.h); no device, no liborbhip
//   otherwise          the class runs on liborbhip, the reference is ORBmatcher::SearchBySim3 (the path before the entry point)
// Then the three ways the class says "not here" (-1, vpMatches12 untouched): a key frame without a row, a point that was never Put,
// and -- on the mock -- a device call that fails.
// Prints "ok <agreed> <one-sided 0> <one-sided 1> <digest>" and returns 0, or the failed checks.  The digest is over the return
// value and vpMatches12, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "ref_sim3.h"
#ifndef SIM3SEARCH_MOCK
#include "ORBmatcher.h"
#else
extern "C" int mock_sim3_calls();
extern "C" void mock_sim3_fail_next();
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

static const int W = 376, H = 241, NLEVELS = 8, NLM = 300;
static const float S = 1.2f, FX = 300.f, CX = 188.f, CY = 120.5f, S12 = 1.37f;

struct World {
    std::vector<KeyFrame *> kfs;                 // the two sides of the loop
    std::vector<MapPoint *> pts;
    std::vector<MapPoint *> matches12;           // what SearchByBoW left
    cv::Mat R12, t12;
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

static KeyFrame *new_keyframe(int k)
{
    KeyFrame *kf = new KeyFrame();
    const float a = 0.03f * (k + 1), c = cosf(a), s = sinf(a);
    const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, C[3] = {0.3f * k - 0.2f, 0.05f * k, 0.1f * k};
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
    return kf;
}

// camera coordinates -> world, through the key frame's own pose
static void to_world(KeyFrame *kf, const double pc[3], float out[3])
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int q = 0; q < 3; q++) s += (double)kf->Tcw.at<float>(q, r) * (pc[q] - (double)kf->Tcw.at<float>(q, 3));
        out[r] = (float)s;
    }
}

static void build(World &Wd)
{
    g_seed = 9151;
    const float a = 0.02f;
    const float R[9] = {cosf(a), 0, sinf(a), 0, 1, 0, -sinf(a), 0, cosf(a)}, t[3] = {0.15f, -0.05f, 0.3f};
    Wd.R12 = cv::Mat(3, 3, CV_32F), Wd.t12 = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Wd.R12.at<float>(r, c) = R[3 * r + c];
        Wd.t12.at<float>(r, 0) = t[r];
    }
    for (int k = 0; k < 2; k++) Wd.kfs.push_back(new_keyframe(k));
    std::vector<std::vector<uint8_t> > rows(2);
    std::vector<int> featOf[2] = {std::vector<int>(NLM, -1), std::vector<int>(NLM, -1)};
    std::vector<std::vector<float> > world[2] = {std::vector<std::vector<float> >(NLM), std::vector<std::vector<float> >(NLM)};
    for (int j = 0; j < NLM + 60; j++) {
        uint8_t base[32];
        for (int b = 0; b < 32; b++) base[b] = (uint8_t)rnd(256);
        const float angle = frand(0, 350);
        // the landmark in camera 1, and where the similarity puts it in camera 2: p2 = (1 / s12) R12' (p1 - t12)
        const double p1[3] = {frand(-3.5f, 3.5f), frand(-2.2f, 2.2f), frand(3.5f, 11.f)};
        double p2[3];
        for (int r = 0; r < 3; r++) {
            double s = 0;
            for (int q = 0; q < 3; q++) s += (double)Wd.R12.at<float>(q, r) * (p1[q] - (double)Wd.t12.at<float>(q, 0));
            p2[r] = s / (double)S12;
        }
        const double *pc[2] = {p1, p2};
        for (int k = 0; k < 2; k++) {
            KeyFrame *kf = Wd.kfs[k];
            cv::KeyPoint kp;
            uint8_t d[32];
            if (j < NLM) {
                const float u = FX * (float)(pc[k][0] / pc[k][2]) + CX + frand(-0.5f, 0.5f), v = FX * (float)(pc[k][1] / pc[k][2]) + CY + frand(-0.5f, 0.5f);
                if (u < 2 || u > W - 3 || v < 2 || v > H - 3) continue;
                const float dist = (float)sqrt(pc[k][0] * pc[k][0] + pc[k][1] * pc[k][1] + pc[k][2] * pc[k][2]);
                int oct = (int)floorf(logf(12.f / dist) / logf(S));
                oct = oct < 0 ? 0 : oct > NLEVELS - 1 ? NLEVELS - 1 : oct;
                kp = cv::KeyPoint(u, v, 31.f * powf(S, (float)oct), angle, 50.f, oct, -1);
                memcpy(d, base, 32);
                flip(d, j % 11 == 5 ? 70 : 6);             // some pairs beyond TH_HIGH
                featOf[k][j] = (int)kf->mvKeys.size();
                world[k][j].resize(3);
                to_world(kf, pc[k], world[k][j].data());
            } else {
                kp = cv::KeyPoint(frand(2, W - 3), frand(2, H - 3), 31.f, frand(0, 360), 20.f, (int)rnd(NLEVELS), -1);
                for (int b = 0; b < 32; b++) d[b] = (uint8_t)rnd(256);
            }
            kf->mvKeys.push_back(kp);
            rows[k].insert(rows[k].end(), d, d + 32);
        }
    }
    for (int k = 0; k < 2; k++) {
        KeyFrame *kf = Wd.kfs[k];
        kf->mvKeysUn = kf->mvKeys;
        kf->N = (int)kf->mvKeys.size();
        kf->mDescriptors = cv::Mat(kf->N, 32, CV_8U);
        memcpy(kf->mDescriptors.ptr(0), rows[k].data(), rows[k].size());
        kf->mvpMapPoints.assign(kf->N, (MapPoint *)NULL);
    }
    // each side's own points: seven landmarks in ten hold one, independently per side
    std::vector<MapPoint *> pointOf[2] = {std::vector<MapPoint *>(NLM, (MapPoint *)NULL), std::vector<MapPoint *>(NLM, (MapPoint *)NULL)};
    for (int j = 0; j < NLM; j++)
        for (int k = 0; k < 2; k++)
            if (featOf[k][j] >= 0 && rnd(10) < 7)
                hold(Wd.kfs[k], featOf[k][j], pointOf[k][j] = new_point(Wd, world[k][j].data(), &rows[k][(size_t)featOf[k][j] * 32]));
    // what SearchByBoW left: every ninth landmark that both sides hold is matched already
    Wd.matches12.assign(Wd.kfs[0]->N, (MapPoint *)NULL);
    for (int j = 0; j < NLM; j += 9)
        if (pointOf[0][j] && pointOf[1][j]) Wd.matches12[featOf[0][j]] = pointOf[1][j];
    for (size_t i = 5; i < Wd.pts.size(); i += 31) Wd.pts[i]->SetBadFlag();   // bad points that their key frames still hold
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
static std::vector<int> indices(const World &Wd, const std::vector<MapPoint *> &v)
{
    std::vector<int> out;
    for (size_t i = 0; i < v.size(); i++) out.push_back(index_of(Wd, v[i]));
    return out;
}

int main()
{
    World A, B, C;
    build(A);
    build(B);
    build(C);
    const float th = 7.5f;                               // ref: src/LoopClosing.cc:375
    // what the scene holds, by the host restatement alone
    refsim3::Stats st;
    std::vector<MapPoint *> mC = C.matches12;
    const int nC = refsim3::SearchBySim3(C.kfs[0], C.kfs[1], mC, S12, C.R12, C.t12, th, &st);
    int pre = 0, bad = 0;
    for (size_t i = 0; i < C.matches12.size(); i++) pre += C.matches12[i] ? 1 : 0;
    for (size_t i = 0; i < C.pts.size(); i++) bad += C.pts[i]->isBad() ? 1 : 0;
    printf("# features %d / %d, points %d (bad %d), matched before %d; active %d / %d, agreed %d, one-sided %d / %d\n", C.kfs[0]->N, C.kfs[1]->N,
           (int)C.pts.size(), bad, pre, st.active0, st.active1, nC, st.oneSided0, st.oneSided1);
    CHECK(nC >= 20 && st.oneSided0 >= 1 && st.oneSided1 >= 1 && pre >= 5 && bad >= 5 && C.pts.size() >= 300);

    std::vector<MapPoint *> mA = A.matches12, mB = B.matches12;
    int nA = 0, nB = 0;
    {
        LocalMapSearch LS(4096);
        LS.InitKeyFrames(16, 1024);
        LS.Put(A.pts);
        LS.PutKeyFrame(A.kfs[0]);
        LS.PutKeyFrame(A.kfs[1]);
        nA = LS.SearchBySim3(A.kfs[0], A.kfs[1], mA, S12, A.R12, A.t12, th);
#ifdef SIM3SEARCH_MOCK
        nB = refsim3::SearchBySim3(B.kfs[0], B.kfs[1], mB, S12, B.R12, B.t12, th);
#else
        ORBmatcher matcher(0.75f, true);                 // ref: src/LoopClosing.cc:246
        nB = matcher.SearchBySim3(B.kfs[0], B.kfs[1], mB, S12, B.R12, B.t12, th);
#endif
        CHECK(nA == nB && nA == nC && indices(A, mA) == indices(B, mB) && indices(A, mA) == indices(C, mC));
        CHECK(indices(A, mA) != indices(A, A.matches12));
        mix((unsigned long long)nA);
        for (size_t i = 0; i < mA.size(); i++) mix((unsigned long long)(index_of(A, mA[i]) + 2));
        // a second call on what the first left: everything agreed is taken now, nothing new agrees
        std::vector<MapPoint *> again = mA;
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], again, S12, A.R12, A.t12, th) == 0 && again == mA);
        CHECK(OrbHipErrorCount() == 0);

        // ---- "not here": -1 and vpMatches12 untouched ----
        // a point that was never Put, held by key frame 2
        int freeFeat = -1;
        for (int i = 0; i < A.kfs[1]->N && freeFeat < 0; i++)
            if (!A.kfs[1]->mvpMapPoints[i]) freeFeat = i;
        CHECK(freeFeat >= 0);
        const float P[3] = {0.f, 0.f, 5.f};
        MapPoint *stranger = new_point(A, P, A.kfs[1]->mDescriptors.ptr(freeFeat));
        hold(A.kfs[1], freeFeat, stranger);
        std::vector<MapPoint *> m = A.matches12;
#ifdef SIM3SEARCH_MOCK
        const int calls = mock_sim3_calls();
#endif
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], m, S12, A.R12, A.t12, th) == -1 && m == A.matches12);
        stranger->SetBadFlag();                          // a bad point the store does not know is nobody's business
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], m, S12, A.R12, A.t12, th) == nA && m == mA);
        m = A.matches12;
#ifdef SIM3SEARCH_MOCK
        CHECK(mock_sim3_calls() == calls + 1);           // the first of the two never reached the device
        CHECK(OrbHipErrorCount() == 0);
        mock_sim3_fail_next();                           // the device call fails
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], m, S12, A.R12, A.t12, th) == -1 && m == A.matches12);
        CHECK(OrbHipErrorCount() == 1);
#endif
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], m, S12, A.R12, A.t12, th) == nA && m == mA);
    }
    {   // a key frame without a row
        LocalMapSearch LS(4096);
        LS.InitKeyFrames(16, 1024);
        LS.Put(A.pts);
        LS.PutKeyFrame(A.kfs[0]);
        std::vector<MapPoint *> m = A.matches12;
        CHECK(LS.SearchBySim3(A.kfs[0], A.kfs[1], m, S12, A.R12, A.t12, th) == -1 && m == A.matches12);
        CHECK(LS.SearchBySim3(A.kfs[1], A.kfs[0], m, S12, A.R12, A.t12, th) == -1 && m == A.matches12);
    }
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %d %d %016llx\n", nA, st.oneSided0, st.oneSided1, g_digest);
    return 0;
}
