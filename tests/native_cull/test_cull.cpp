// test_cull.cpp -- ORB_SLAM2::LocalMapSearch::KeyFrameCulling on mock KeyFrame / MapPoint objects against the sequential loop of
// ref_cull.h on a twin map built from the same seed.
//   main scene   30 key frames, 1200 points seen from 4 to 9 neighbouring key frames at octaves 0..4, a third of the features
//                stereo, some of them far; run monocular and not, with a skip functor that reads what the previous cull changed.
//                Compared: the culled key frames in order, isBad() and Observations() of every point, every key frame's
//                mvpMapPoints, and afterwards the counts of every surviving key frame (the resident state followed the culls).
//                One point is never Put: its observers go the host way.  The key frame with mnId 0 is as redundant as any.
//   scene A      culling A takes the third other observer from B's points: B stays, though one batch at the start says cull
//   scene B      culling A turns two points of B bad: B goes, though one batch at the start says keep
//   -DCULL_MOCK  the class runs on the host model of the entry points (mock_cull.cc); no device, no liborbhip
//   otherwise    the class runs on liborbhip
// Prints "ok <culled> <key frames counted the device way> <the host way> <digest>" and returns 0, or the failed checks.  The digest is
// over every compared value, so the two programs must print the same line.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_cull.h"

using namespace ORB_SLAM2;

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

// a key frame of n features, all at `octave`, monocular and near, until the caller says otherwise
static KeyFrame *new_kf(World &W, int n, int octave = 0)
{
    KeyFrame *kf = new KeyFrame();
    kf->mnId = W.kfs.size();     // the same ids in both maps (the constructor counts across them)
    kf->N = n;
    kf->mvpMapPoints.assign(n, (MapPoint *)NULL);
    kf->mvKeysUn.resize(n);
    for (int i = 0; i < n; i++) kf->mvKeysUn[i].octave = octave;
    kf->mvuRight.assign(n, -1.f);
    kf->mvDepth.assign(n, -1.f);
    kf->mThDepth = 40.f;
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
    const int idx = W.nextFree[k]++;
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
    if (!p->mpRefKF) p->mpRefKF = kf;
    return true;
}

// ---- the class's side: what the integrator tells LocalMapSearch ----
struct Resident {
    LocalMapSearch LS;
    Resident(World &A, MapPoint *never = NULL, int leaveOut = -1) : LS(4096)
    {
        LS.InitKeyFrames(64, 512);
        std::vector<MapPoint *> v;
        for (size_t i = 0; i < A.pts.size(); i++)
            if (A.pts[i] != never) v.push_back(A.pts[i]);
        LS.Put(v);
        for (size_t k = 0; k < A.kfs.size(); k++)
            if ((int)k != leaveOut) LS.PutKeyFrame(A.kfs[k]);      // (one key frame may be left for the class to put)
    }
};

static std::vector<long> ids(const std::vector<KeyFrame *> &v)
{
    std::vector<long> out;
    for (size_t i = 0; i < v.size(); i++) out.push_back((long)v[i]->mnId);
    return out;
}

// the two maps after the loops, by mnId
static void compare(World &A, World &B)
{
    bool bad = true, obs = true, rows = true, kfbad = true;
    CHECK(A.pts.size() == B.pts.size() && A.kfs.size() == B.kfs.size());
    for (size_t j = 0; j < A.pts.size(); j++) {
        bad = bad && A.pts[j]->isBad() == B.pts[j]->isBad();
        obs = obs && A.pts[j]->Observations() == B.pts[j]->Observations() && A.pts[j]->mObservations.size() == B.pts[j]->mObservations.size();
        mix(((unsigned long long)A.pts[j]->Observations() << 1) | (A.pts[j]->isBad() ? 1u : 0u));
    }
    for (size_t k = 0; k < A.kfs.size(); k++) {
        kfbad = kfbad && A.kfs[k]->isBad() == B.kfs[k]->isBad();
        for (int i = 0; i < A.kfs[k]->N; i++) {
            MapPoint *a = A.kfs[k]->mvpMapPoints[i], *b = B.kfs[k]->mvpMapPoints[i];
            rows = rows && (a ? (long)a->mnId : -1) == (b ? (long)b->mnId : -1);
            mix((unsigned long long)(a ? (long)a->mnId : -1));
        }
    }
    CHECK(bad);
    CHECK(obs);
    CHECK(rows);
    CHECK(kfbad);
}

static long g_culled = 0;

// the counts of every surviving key frame: the class on map A (device, on the table the culls left) against the loop on map B
static void compare_counts(Resident &R, World &A, World &B, bool bMonocular)
{
    std::vector<KeyFrame *> va, vb;
    for (size_t k = 0; k < A.kfs.size(); k++)
        if (!A.kfs[k]->isBad()) va.push_back(A.kfs[k]), vb.push_back(B.kfs[k]);
    std::vector<LocalMapSearch::CullCount> c;
    CHECK(R.LS.CullCounts(va, bMonocular, c) && c.size() == va.size());
    bool same = true;
    for (size_t k = 0; k < c.size(); k++) {
        const refcull::Count r = refcull::count(vb[k], bMonocular);
        same = same && c[k].nMPs == r.nMPs && c[k].nRedundant == r.nRedundant && c[k].bRedundant == r.bRedundant;
        mix(((unsigned long long)c[k].nMPs << 32) | (unsigned)(c[k].nRedundant << 1) | (c[k].bRedundant ? 1u : 0u));
    }
    CHECK(same);
}

struct Never {
    bool operator()(KeyFrame *) const { return false; }
};
// skips a key frame while the one before it (mnId - 1) is bad: state that the previous cull of the same loop changed
struct AfterACull {
    World *W;
    long *asked, *skipped;
    bool operator()(KeyFrame *pKF) const
    {
        ++*asked;
        const bool skip = pKF->mnId > 0 && W->kfs[pKF->mnId - 1]->isBad();
        *skipped += skip ? 1 : 0;
        return skip;
    }
};
struct SetBad {
    std::vector<KeyFrame *> *culled;
    void operator()(KeyFrame *pKF) const
    {
        pKF->SetBadFlag();
        culled->push_back(pKF);
    }
};

template <class SkipA, class SkipB>
static std::vector<long> run_both(Resident &R, World &A, World &B, const std::vector<int> &order, bool bMonocular, SkipA skipA, SkipB skipB)
{
    std::vector<KeyFrame *> va, vb, culledA;
    for (size_t i = 0; i < order.size(); i++) va.push_back(A.kfs[order[i]]), vb.push_back(B.kfs[order[i]]);
    const std::vector<KeyFrame *> culledB = refcull::KeyFrameCulling(vb, bMonocular, skipB);
    const SetBad cull = {&culledA};
    const int n = R.LS.KeyFrameCulling(va, bMonocular, skipA, cull);
    CHECK(n == (int)culledA.size());
    CHECK(ids(culledA) == ids(culledB));
    for (size_t i = 0; i < culledA.size(); i++) mix((unsigned long long)culledA[i]->mnId);
    g_culled += n;
    compare(A, B);
    return ids(culledA);
}

// ---- the main scene ----
static const int NKF = 30, NPT = 1200, NFEAT = 420, WINDOW = 5;

static MapPoint *build(World &W, unsigned seed)
{
    g_seed = seed;
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new_kf(W, NFEAT);
        for (int i = 0; i < NFEAT; i++) {
            const unsigned o = rnd(10);                          // most features at octaves 1 and 2, some finer, some coarser
            kf->mvKeysUn[i].octave = o == 0 ? 0 : o == 1 ? 3 + (int)rnd(2) : 1 + (int)rnd(2);
            if (rnd(3) == 0) {                                   // a stereo feature; one in six of them far
                kf->mvuRight[i] = 10.f;
                kf->mvDepth[i] = rnd(6) == 0 ? 55.f : 12.f;
            }
        }
    }
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new_point(W);
        const int n = 4 + (int)rnd(6), centre = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 200; tries++) {
            const int k = centre - WINDOW + (int)rnd(2 * WINDOW + 1);
            if (k >= 0 && k < NKF) observe(W, p, k);
        }
    }
    MapPoint *never = new_point(W);                              // never Put: key frames 4, 5, 6 go the host way
    observe(W, never, 4), observe(W, never, 5), observe(W, never, 6);
    return never;
}

static void main_scene(unsigned seed, bool bMonocular, bool withSkip)
{
    World A, B;
    MapPoint *never = build(A, seed);
    build(B, seed);
    Resident R(A, never, withSkip ? -1 : 17);   // (a key frame the functor skips first would never be put: every observer needs its row)
    std::vector<int> order;
    for (int k = 0; k < NKF; k++) order.push_back(k);
    g_seed = seed + 1;
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rnd((unsigned)i)]);
    const long deviceBefore = LocalMapSearch::CullWayCounts().device, hostBefore = LocalMapSearch::CullWayCounts().host;
    std::vector<long> culled;
    long askedA = 0, askedB = 0, skippedA = 0, skippedB = 0;
    if (withSkip) {
        const AfterACull sa = {&A, &askedA, &skippedA}, sb = {&B, &askedB, &skippedB};
        culled = run_both(R, A, B, order, bMonocular, sa, sb);
        CHECK(askedA == askedB && askedA == NKF - 1);
        CHECK(skippedA == skippedB && skippedA > 0);
        for (size_t i = 0; i < culled.size(); i++)               // no two neighbours in mnId went, though both were candidates
            CHECK(std::find(culled.begin(), culled.end(), culled[i] + 1) == culled.end() ||
                  std::find(culled.begin(), culled.end(), culled[i] + 1) < std::find(culled.begin(), culled.end(), culled[i]));
    } else {
        culled = run_both(R, A, B, order, bMonocular, Never(), Never());
    }
    printf("# seed %u monocular %d skip %d: %d culled\n", seed, (int)bMonocular, (int)withSkip, (int)culled.size());
    CHECK(culled.size() >= 3 && culled.size() <= 20);
    CHECK(!A.kfs[0]->isBad() && std::find(culled.begin(), culled.end(), 0L) == culled.end());
    CHECK(LocalMapSearch::CullWayCounts().device > deviceBefore && LocalMapSearch::CullWayCounts().host > hostBefore);
    long turned = 0;
    for (size_t j = 0; j < A.pts.size(); j++) turned += A.pts[j]->isBad() ? 1 : 0;
    mix((unsigned long long)turned);
    compare_counts(R, A, B, bMonocular);
    compare_counts(R, A, B, !bMonocular);
}

// ---- the two scenes that say why the candidates are counted again after a cull ----
static void fill(World &W, int k, const std::vector<int> &pts)
{
    for (size_t i = 0; i < pts.size(); i++) CHECK(observe(W, W.pts[pts[i]], k));
}
static std::vector<int> range(int a, int b)
{
    std::vector<int> v;
    for (int i = a; i < b; i++) v.push_back(i);
    return v;
}
static std::vector<int> cat(std::vector<int> a, const std::vector<int> &b)
{
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

static void build_scene_a(World &W)
{   // key frames 1..4 = A, B, C, D all see points 0..9 (0 is the key frame with mnId 0 and sees nothing)
    for (int k = 0; k < 5; k++) new_kf(W, 16);
    for (int j = 0; j < 10; j++) new_point(W);
    for (int k = 1; k < 5; k++) fill(W, k, range(0, 10));
}

static void build_scene_b(World &W)
{   // S = 0..19, Q = 20..29, W = 30, 31; key frames 1..6 = A, B, C, D, E, F
    for (int k = 0; k < 7; k++) new_kf(W, 32);
    for (int j = 0; j < 32; j++) new_point(W);
    const std::vector<int> S = range(0, 20), Q = range(20, 30), Wp = range(30, 32);
    fill(W, 1, cat(S, Wp));
    fill(W, 2, cat(Q, Wp));
    for (int k = 3; k < 6; k++) fill(W, k, cat(S, Q));
    fill(W, 6, Wp);
}

static void hand_scene(void (*build_scene)(World &), bool bAtStart, const std::vector<long> &expected, const int countsAtStart[4])
{
    World A, B;
    build_scene(A);
    build_scene(B);
    Resident R(A);
    std::vector<KeyFrame *> cands;
    cands.push_back(A.kfs[1]), cands.push_back(A.kfs[2]);
    std::vector<LocalMapSearch::CullCount> c;
    CHECK(R.LS.CullCounts(cands, true, c) && c.size() == 2);
    if (c.size() == 2) {
        CHECK(c[0].nMPs == countsAtStart[0] && c[0].nRedundant == countsAtStart[1] && c[0].bRedundant);
        CHECK(c[1].nMPs == countsAtStart[2] && c[1].nRedundant == countsAtStart[3]);
        CHECK(c[1].bRedundant == bAtStart);                       // what one batch at the start says of B ...
    }
    std::vector<int> order;
    order.push_back(0), order.push_back(1), order.push_back(2);
    const std::vector<long> culled = run_both(R, A, B, order, true, Never(), Never());
    CHECK(culled == expected);                                    // ... and what the sequence does
    CHECK((std::find(culled.begin(), culled.end(), 2L) != culled.end()) != bAtStart);
    compare_counts(R, A, B, true);
}

int main()
{
    {
        const int atStart[4] = {10, 10, 10, 10};
        hand_scene(build_scene_a, true, std::vector<long>(1, 1L), atStart);
    }
    {
        const int atStart[4] = {22, 20, 12, 10};
        std::vector<long> both;
        both.push_back(1), both.push_back(2);
        hand_scene(build_scene_b, false, both, atStart);
    }
    main_scene(4711, true, false);
    main_scene(4712, false, false);
    main_scene(4713, true, true);

    const long dev = LocalMapSearch::CullWayCounts().device, host = LocalMapSearch::CullWayCounts().host;
    CHECK(dev > 100 && host > 3);
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %ld %ld %ld %016llx\n", g_culled, dev, host, g_digest);
    return 0;
}
