// test_baproblem.cpp -- ORB_SLAM2::LocalMapSearch::BuildLocalBA / BuildBAProblem on mock KeyFrame / MapPoint objects against the
// three loops of ref_ba.h on a twin map built from the same seed.
//   the map      12 key frames of 640 features, 1500 points seen from 3 to 7 neighbouring key frames; the covisibility lists by
//                hand.  After the map is resident: one point turns bad, one key frame is culled (SetBadFlag: its observations go,
//                points left with two observers turn bad, its row is erased) and stays in its neighbours' covisibility lists.
//   compared     the five vectors (by mnId and index) and, on every key frame and point, mnBALocalForKF / mnBAFixedForKF:
//                every key frame's BuildLocalBA, a window of six in the caller's order with one key frame twice, a bad and a NULL
//                entry, and every key frame at once (the global problem: nothing is fixed; its edges exceed the first offer of
//                room, so the call is made twice)
//   false        a local key frame without a row; with -DBA_MOCK also a failing entry point: `out` stays empty both times
//   -DBA_MOCK    the class runs on the host model of the entry points (mock_ba.cc); no device, no liborbhip
//   otherwise    the class runs on liborbhip
// Prints "ok <problems> <edges> <digest>" and returns 0, or the failed checks.  The digest is over every compared value, so the
// two programs must print the same line.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_ba.h"

using namespace ORB_SLAM2;

#ifdef BA_MOCK
void mock_ba_fail(int on);
long mock_ba_calls();
#endif

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

struct World {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> pts;
    std::vector<int> nextFree;   // the next feature of each key frame that holds no point
    ~World()
    {
        for (size_t i = 0; i < pts.size(); i++) delete pts[i];
        for (size_t i = 0; i < kfs.size(); i++) delete kfs[i];
    }
};

static KeyFrame *new_kf(World &W, int n)
{
    KeyFrame *kf = new KeyFrame();
    kf->mnId = W.kfs.size();     // the same ids in both maps (the constructor counts across them)
    kf->N = n;
    kf->mvpMapPoints.assign(n, (MapPoint *)NULL);
    kf->mvKeysUn.resize(n);
    kf->mvuRight.assign(n, -1.f);
    kf->mvDepth.assign(n, -1.f);
    W.kfs.push_back(kf);
    W.nextFree.push_back(0);
    return kf;
}

static MapPoint *new_point(World &W)
{
    MapPoint *p = new MapPoint();
    p->mnId = W.pts.size();
    p->mWorldPos = cv::Mat::zeros(3, 1, CV_32F), p->mNormalVector = cv::Mat::zeros(3, 1, CV_32F), p->mDescriptor = cv::Mat::zeros(1, 32, CV_8U);
    p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
    W.pts.push_back(p);
    return p;
}

static bool observe(World &W, MapPoint *p, int k)
{
    KeyFrame *kf = W.kfs[k];
    if (p->IsInKeyFrame(kf) || W.nextFree[k] >= kf->N) return false;
    const int idx = W.nextFree[k];
    W.nextFree[k] += rnd(4) == 0 ? 2 : 1;      // (empty features in between)
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
    if (!p->mpRefKF) p->mpRefKF = kf;
    return true;
}

static const int NKF = 12, NPT = 1500, NFEAT = 640, WINDOW = 3, CULLED = 5, BADPOINT = 77;

static void build(World &W, unsigned seed)
{
    g_seed = seed;
    for (int k = 0; k < NKF; k++) new_kf(W, NFEAT);
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new_point(W);
        const int n = 3 + (int)rnd(5), centre = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 200; tries++) {
            const int k = centre - WINDOW + (int)rnd(2 * WINDOW + 1);
            if (k >= 0 && k < NKF) observe(W, p, k);
        }
    }
    for (int k = 0; k < NKF; k++) {                 // the covisibility lists: the two key frames on either side, nearest last
        static const int order[4] = {2, -2, -1, 1};
        for (int o = 0; o < 4; o++)
            if (k + order[o] >= 0 && k + order[o] < NKF) W.kfs[k]->mvpOrderedConnectedKeyFrames.push_back(W.kfs[k + order[o]]);
    }
}

// the edits both maps get after the class has seen map A; returns the culled key frame's points from before
static std::vector<MapPoint *> edit(World &W)
{
    W.pts[BADPOINT]->SetBadFlag();             // (the flag alone: its observers keep it)
    const std::vector<MapPoint *> its = W.kfs[CULLED]->GetMapPointMatches();
    W.kfs[CULLED]->SetBadFlag();
    return its;
}

// The reference's walks read the stamps of earlier runs (a point stamped with this run's id is not taken again); the class reads
// none.  Every run starts from stamps no id equals, on both maps.
static void reset_stamps(World &W)
{
    for (size_t k = 0; k < W.kfs.size(); k++) W.kfs[k]->mnBALocalForKF = W.kfs[k]->mnBAFixedForKF = ~0ul;
    for (size_t j = 0; j < W.pts.size(); j++) W.pts[j]->mnBALocalForKF = ~0ul;
}

template <class P> static long id_of(P *p) { return p ? (long)p->mnId : -1; }

// the five vectors of the class's problem on map A against the loops' on map B, and every stamp of the two maps
template <class A, class B> static void compare(const A &a, const B &b, World &WA, World &WB)
{
    CHECK(a.vpLocalKFs.size() == b.vpLocalKFs.size() && a.vpFixedKFs.size() == b.vpFixedKFs.size());
    CHECK(a.vpLocalMPs.size() == b.vpLocalMPs.size() && a.vEdges.size() == b.vEdges.size());
    CHECK(a.vEdgeOff.size() == b.vEdgeOff.size() && a.vEdgeOff.size() == a.vpLocalMPs.size() + 1);
    bool kfs = true, fixed = true, pts = true, off = true, edges = true, stamps = true;
    for (size_t i = 0; i < a.vpLocalKFs.size() && i < b.vpLocalKFs.size(); i++) kfs = kfs && id_of(a.vpLocalKFs[i]) == id_of(b.vpLocalKFs[i]);
    for (size_t i = 0; i < a.vpFixedKFs.size() && i < b.vpFixedKFs.size(); i++) {
        fixed = fixed && id_of(a.vpFixedKFs[i]) == id_of(b.vpFixedKFs[i]) && a.vpFixedKFs[i] == WA.kfs[a.vpFixedKFs[i]->mnId];
        mix((unsigned long long)id_of(a.vpFixedKFs[i]));
    }
    for (size_t i = 0; i < a.vpLocalMPs.size() && i < b.vpLocalMPs.size(); i++) {
        pts = pts && id_of(a.vpLocalMPs[i]) == id_of(b.vpLocalMPs[i]) && a.vpLocalMPs[i] == WA.pts[a.vpLocalMPs[i]->mnId];
        mix((unsigned long long)id_of(a.vpLocalMPs[i]));
    }
    for (size_t i = 0; i < a.vEdgeOff.size() && i < b.vEdgeOff.size(); i++) off = off && a.vEdgeOff[i] == b.vEdgeOff[i];
    for (size_t i = 0; i < a.vEdges.size() && i < b.vEdges.size(); i++) {
        edges = edges && id_of(a.vEdges[i].pKF) == id_of(b.vEdges[i].pKF) && a.vEdges[i].idx == b.vEdges[i].idx &&
                a.vEdges[i].pKF == WA.kfs[a.vEdges[i].pKF->mnId];
        mix(((unsigned long long)id_of(a.vEdges[i].pKF) << 32) | (unsigned long long)a.vEdges[i].idx);
    }
    for (size_t k = 0; k < WA.kfs.size(); k++) {
        stamps = stamps && WA.kfs[k]->mnBALocalForKF == WB.kfs[k]->mnBALocalForKF && WA.kfs[k]->mnBAFixedForKF == WB.kfs[k]->mnBAFixedForKF;
        mix(((unsigned long long)WA.kfs[k]->mnBALocalForKF << 32) | WA.kfs[k]->mnBAFixedForKF);
    }
    for (size_t j = 0; j < WA.pts.size(); j++) {
        stamps = stamps && WA.pts[j]->mnBALocalForKF == WB.pts[j]->mnBALocalForKF;
        mix((unsigned long long)WA.pts[j]->mnBALocalForKF);
    }
    CHECK(kfs);
    CHECK(fixed);
    CHECK(pts);
    CHECK(off);
    CHECK(edges);
    CHECK(stamps);
}

static bool is_empty(const LocalMapSearch::BAProblem &p)
{
    return p.vpLocalKFs.empty() && p.vpFixedKFs.empty() && p.vpLocalMPs.empty() && p.vEdgeOff.empty() && p.vEdges.empty();
}

int main()
{
    World A, B;
    build(A, 2024);
    build(B, 2024);
    LocalMapSearch LS(4096);
    LS.InitKeyFrames(64, 1024);
    LS.Put(A.pts);
    for (int k = 0; k < NKF; k++) LS.PutKeyFrame(A.kfs[k]);

    // ---- the edits, told to the class as INTEGRATION.md section 3e says ----
    const std::vector<MapPoint *> its = edit(A);
    edit(B);
    LS.UpdateFlags(A.pts[BADPOINT]);
    LS.EraseKeyFrame(A.kfs[CULLED]);
    long turned = 0;
    for (size_t i = 0; i < its.size(); i++)
        if (its[i] && its[i]->isBad()) LS.UpdateFlags(its[i]), turned++;
    CHECK(turned > 0 && A.kfs[CULLED]->isBad());
    mix((unsigned long long)turned);

    long problems = 0, edgesTotal = 0;
    LocalMapSearch::BAProblem out;
    refba::Problem ref;

    // ---- every key frame at once: the global problem ----
    {
        reset_stamps(A), reset_stamps(B);
        std::vector<KeyFrame *> va(A.kfs.begin(), A.kfs.end());
        std::list<KeyFrame *> lb;
        for (int k = 0; k < NKF; k++)
            if (!B.kfs[k]->isBad()) lb.push_back(B.kfs[k]), B.kfs[k]->mnBALocalForKF = B.kfs[NKF - 1]->mnId;
        refba::Build(lb, B.kfs[NKF - 1]->mnId, ref);
#ifdef BA_MOCK
        const long before = mock_ba_calls();
#endif
        CHECK(LS.BuildBAProblem(va, out));
#ifdef BA_MOCK
        CHECK(mock_ba_calls() == before + 2);      // more than 4096 edges: the first offer of room was too small
#endif
        CHECK(out.vpFixedKFs.empty() && out.vEdges.size() > 4096 && (int)out.vpLocalKFs.size() == NKF - 1);
        compare(out, ref, A, B);
        problems++, edgesTotal += (long)out.vEdges.size();
    }
    // ---- LocalBundleAdjustment of every key frame ----
    bool sawFixed = false, sawBadNeighbour = false;
    for (int k = 0; k < NKF; k++) {
        if (A.kfs[k]->isBad()) continue;
        reset_stamps(A), reset_stamps(B);
        refba::Build(refba::LocalKeyFrames(B.kfs[k]), B.kfs[k]->mnId, ref);
        CHECK(LS.BuildLocalBA(A.kfs[k], out));
        compare(out, ref, A, B);
        sawFixed = sawFixed || out.vpFixedKFs.size() >= 2;
        sawBadNeighbour = sawBadNeighbour || out.vpLocalKFs.size() < A.kfs[k]->mvpOrderedConnectedKeyFrames.size() + 1;
        bool every = true;
        for (size_t j = 0; j + 1 < out.vEdgeOff.size(); j++) every = every && out.vEdgeOff[j + 1] > out.vEdgeOff[j];
        CHECK(every && !out.vEdgeOff.empty() && out.vEdgeOff.back() == (int32_t)out.vEdges.size());
        for (size_t i = 0; i < out.vpFixedKFs.size(); i++) CHECK(out.vpFixedKFs[i] != A.kfs[CULLED]);
        problems++, edgesTotal += (long)out.vEdges.size();
    }
    CHECK(sawFixed && sawBadNeighbour);
    // ---- a window in the caller's order: one key frame twice, the bad one and a NULL in between ----
    {
        static const int win[8] = {8, 3, 6, CULLED, 3, -1, 4, 7};
        reset_stamps(A), reset_stamps(B);
        std::vector<KeyFrame *> va;
        std::list<KeyFrame *> lb;
        for (int i = 0; i < 8; i++) {
            va.push_back(win[i] < 0 ? (KeyFrame *)NULL : A.kfs[win[i]]);
            if (win[i] >= 0 && !B.kfs[win[i]]->isBad()) lb.push_back(B.kfs[win[i]]), B.kfs[win[i]]->mnBALocalForKF = B.kfs[7]->mnId;
        }
        refba::Build(lb, B.kfs[7]->mnId, ref);
        CHECK(LS.BuildBAProblem(va, out));
        CHECK(out.vpLocalKFs.size() == 6 && !out.vpFixedKFs.empty());
        compare(out, ref, A, B);
        problems++, edgesTotal += (long)out.vEdges.size();
    }
    // ---- false: a local key frame without a row; a failing entry point ----
    unsigned long expectedErrors = 0;
    {
        World C;
        KeyFrame *stranger = new KeyFrame();
        stranger->mnId = 1000, stranger->N = 4;      // (no row of the table has this id)
        stranger->mvpMapPoints.assign(4, (MapPoint *)NULL);
        C.kfs.push_back(stranger);
        std::vector<KeyFrame *> v;
        v.push_back(A.kfs[2]), v.push_back(stranger);
        CHECK(LS.BuildBAProblem(v, out) == false && is_empty(out));
        CHECK(LS.BuildLocalBA(stranger, out) == false && is_empty(out));
        CHECK(LS.BuildLocalBA(NULL, out) == false && is_empty(out));
        CHECK(LS.BuildBAProblem(std::vector<KeyFrame *>(), out) == true && is_empty(out));
#ifdef BA_MOCK
        mock_ba_fail(1);
        CHECK(LS.BuildLocalBA(A.kfs[2], out) == false && is_empty(out));
        mock_ba_fail(0);
        expectedErrors = 1;
#endif
        CHECK(LS.BuildLocalBA(A.kfs[2], out) && !is_empty(out));
    }
    CHECK(OrbHipErrorCount() == expectedErrors);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %ld %ld %016llx\n", problems, edgesTotal, g_digest);
    return 0;
}
