// test_bowcand.cpp -- both overloads of ORB_SLAM2::LocalMapSearch::SearchByBoWCandidates on mock KeyFrame / MapPoint / Frame objects:
// 30 key frames of 300 features over 40 vocabulary nodes, 1200 points, a frame; between rounds the map is edited -- Replace,
// SetBadFlag of points, an erased key frame, a bad candidate, a point that was never Put (its key frames go the host way).  The
// map is built twice from one seed: the class works on one copy, the loops of ref_bowcand.h -- per-candidate SearchByBoW and the
// PnPsolver-constructor loop -- on the twin, and every vector, count and correspondence is compared.  Descriptors carry 16 random
// bits, so equal distances and the ratio test decide.
//   -DBOWCAND_MOCK  the class runs on the host model of the entry points (mock_bowcand.cc); no device, no liborbhip
//   otherwise       the class runs on liborbhip
// Prints "ok <calls> <candidates the device way> <candidates the host way> <digest>" and returns 0, or the failed checks.  The
// digest is over every compared value, so the two programs must print the same line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_bowcand.h"

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

static const int NKF = 30, NPT = 1200, NFEAT = 300, NNODES = 40, NLEVELS = 8;
static const float ANGLES[6] = {0.f, 12.f, 31.f, 95.5f, 180.5f, 359.f};

struct World {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> pts;
    Frame F;
    ~World()
    {
        for (size_t i = 0; i < pts.size(); i++) delete pts[i];
        for (size_t i = 0; i < kfs.size(); i++) delete kfs[i];
    }
};

// n features: 16 random descriptor bits, an angle of six, an octave, a node of NNODES
static void features(int n, std::vector<cv::KeyPoint> &keys, cv::Mat &desc, DBoW2::FeatureVector &fv)
{
    keys.resize(n);
    desc = cv::Mat::zeros(n, 32, CV_8U);
    fv.clear();
    for (int i = 0; i < n; i++) {
        keys[i].pt.x = (float)rnd(640) + 0.25f, keys[i].pt.y = (float)rnd(480) + 0.5f;
        keys[i].angle = ANGLES[rnd(6)];
        keys[i].octave = (int)rnd(NLEVELS);
        desc.ptr(i)[0] = (unsigned char)rnd(256), desc.ptr(i)[1] = (unsigned char)rnd(256);
    }
    for (int e = 0; e < n; e++) {           // the lists in a shuffled order: neither ascending nor contiguous
        const int i = (e * 7 + 3) % n;      // (7 and 300 are coprime)
        fv[1 + 3 * rnd(NNODES)].push_back((unsigned)i);
    }
}

static MapPoint *new_point(World &W)
{
    MapPoint *p = new MapPoint();
    p->mnId = W.pts.size();
    p->mWorldPos = cv::Mat::zeros(3, 1, CV_32F), p->mNormalVector = cv::Mat::zeros(3, 1, CV_32F), p->mDescriptor = cv::Mat::zeros(1, 32, CV_8U);
    for (int r = 0; r < 3; r++) p->mWorldPos.at<float>(r, 0) = (float)rnd(2000) * 0.01f - 10.f;
    p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
    W.pts.push_back(p);
    return p;
}

static void observe(MapPoint *p, KeyFrame *kf, int idx)
{
    if (kf->isBad() || p->IsInKeyFrame(kf) || kf->mvpMapPoints[idx]) return;
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
}

static void erase_observation(MapPoint *p, KeyFrame *kf)
{
    if (!p->mObservations.count(kf)) return;
    kf->mvpMapPoints[p->mObservations[kf]] = NULL;
    p->mObservations.erase(kf);
    p->nObs--;
}

static void build(World &W)
{
    g_seed = 2718;
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        kf->mnId = k;                        // the same ids in both maps (the constructor counts across them)
        kf->N = NFEAT;
        features(NFEAT, kf->mvKeysUn, kf->mDescriptors, kf->mFeatVec);
        kf->mvKeys = kf->mvKeysUn;
        kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
        W.kfs.push_back(kf);
    }
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new_point(W);
        const int n = 2 + (int)rnd(6);
        for (int t = 0; t < n; t++) observe(p, W.kfs[rnd(NKF)], (int)rnd(NFEAT));
    }
    W.F.mnId = 5000;
    W.F.N = NFEAT;
    features(NFEAT, W.F.mvKeysUn, W.F.mDescriptors, W.F.mFeatVec);
    W.F.mvKeys = W.F.mvKeysUn;
    W.F.mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
    W.F.mnScaleLevels = NLEVELS;
    float s = 1.f;
    for (int l = 0; l < NLEVELS; l++, s *= 1.2f) W.F.mvScaleFactors.push_back(s), W.F.mvLevelSigma2.push_back(s * s);
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }
static unsigned fbits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

// the class's side of the map: what the integrator tells LocalMapSearch
struct Resident {
    LocalMapSearch LS;
    std::set<MapPoint *> put;
    std::vector<std::vector<MapPoint *> > rows;        // every key frame's row as the table has it (empty: no row)
    Resident() : LS(4096) { LS.InitKeyFrames(64, 512); }
    MapPoint *known(MapPoint *p) { return p && put.count(p) ? p : NULL; }
    void noted(KeyFrame *kf)
    {
        if (rows.size() <= kf->mnId) rows.resize(kf->mnId + 1);
        rows[kf->mnId].clear();
        for (int i = 0; i < kf->N; i++) rows[kf->mnId].push_back(known(kf->mvpMapPoints[i]));
    }
    void put_kf(KeyFrame *kf) { LS.PutKeyFrame(kf), noted(kf); }
    void sync(World &A)                                  // SetMapPoint for every entry that changed since the row was last in step
    {
        for (size_t k = 0; k < A.kfs.size(); k++) {
            KeyFrame *kf = A.kfs[k];
            if (kf->isBad()) continue;
            if (rows.size() <= k || rows[k].empty()) {   // (a row the class put by itself)
                noted(kf);
                continue;
            }
            for (int i = 0; i < kf->N; i++)
                if (known(kf->mvpMapPoints[i]) != rows[k][i]) {
                    rows[k][i] = known(kf->mvpMapPoints[i]);
                    LS.SetMapPoint(kf, (size_t)i, rows[k][i]);
                }
        }
    }
};

static std::vector<long> ids(const std::vector<MapPoint *> &v)
{
    std::vector<long> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = v[i] ? (long)v[i]->mnId : -1;
    return out;
}

static int g_calls = 0;
static long g_matches = 0, g_setups = 0;

// Relocalization's loop on the twin against the class on the first map
static void reloc(Resident &R, World &A, World &B, const std::vector<int> &which, int minMatches, float nnratio, bool ori, bool setups)
{
    std::vector<KeyFrame *> va;
    for (size_t i = 0; i < which.size(); i++) va.push_back(A.kfs[which[i]]);
    std::vector<std::vector<MapPoint *> > vv;
    std::vector<int> vn;
    std::vector<RelocCorrespondences> vs;
    R.LS.SearchByBoWCandidates(va, A.F, vv, vn, setups ? &vs : NULL, minMatches, 5.991f, nnratio, ori);
    g_calls++;
    CHECK(vv.size() == which.size() && vn.size() == which.size() && (!setups || vs.size() == which.size()));
    for (size_t i = 0; i < which.size() && vv.size() == which.size(); i++) {
        KeyFrame *kb = B.kfs[which[i]];
        std::vector<MapPoint *> want;
        int n = 0;
        if (!kb->isBad()) n = refbow::SearchByBoW(kb, B.F, want, nnratio, ori);          // ref: src/Tracking.cc:2598-2602
        CHECK(vn[i] == n);
        CHECK(ids(vv[i]) == ids(want));
        g_matches += n;
        mix((unsigned long long)n);
        const std::vector<long> w = ids(want);
        for (size_t f = 0; f < w.size(); f++) mix((unsigned long long)(w[f] + 1) * 131u + f);
        if (!setups || vs.size() != which.size()) continue;
        RelocCorrespondences ref;
        if (!kb->isBad() && n >= minMatches) refbow::PnPSetup(B.F, want, 5.991f, ref);   // ref: :2603-2611
        const RelocCorrespondences &got = vs[i];
        CHECK(got.mvKeyPointIndices == ref.mvKeyPointIndices);
        bool same = got.mvP2D.size() == ref.mvP2D.size() && got.mvP3Dw.size() == ref.mvP3Dw.size() && got.mvMaxError.size() == ref.mvMaxError.size() &&
                    got.mvP2D.size() == ref.mvKeyPointIndices.size() && got.mvP3Dw.size() == got.mvP2D.size() && got.mvMaxError.size() == got.mvP2D.size();
        for (size_t t = 0; same && t < ref.mvP2D.size(); t++) {
            same = fbits(got.mvP2D[t].x) == fbits(ref.mvP2D[t].x) && fbits(got.mvP2D[t].y) == fbits(ref.mvP2D[t].y) &&
                   fbits(got.mvP3Dw[t].x) == fbits(ref.mvP3Dw[t].x) && fbits(got.mvP3Dw[t].y) == fbits(ref.mvP3Dw[t].y) &&
                   fbits(got.mvP3Dw[t].z) == fbits(ref.mvP3Dw[t].z) && fbits(got.mvMaxError[t]) == fbits(ref.mvMaxError[t]);
            mix(((unsigned long long)fbits(ref.mvP3Dw[t].x) << 32) | fbits(ref.mvMaxError[t]));
        }
        CHECK(same);
        g_setups += (long)ref.mvP2D.size();
    }
}

// ComputeSim3's loop
static void loop(Resident &R, World &A, World &B, int cur, const std::vector<int> &which, float nnratio, bool ori)
{
    std::vector<KeyFrame *> va;
    for (size_t i = 0; i < which.size(); i++) va.push_back(A.kfs[which[i]]);
    std::vector<std::vector<MapPoint *> > vv;
    std::vector<int> vn;
    R.LS.SearchByBoWCandidates(A.kfs[cur], va, vv, vn, nnratio, ori);
    g_calls++;
    CHECK(vv.size() == which.size() && vn.size() == which.size());
    for (size_t i = 0; i < which.size() && vv.size() == which.size(); i++) {
        KeyFrame *kb = B.kfs[which[i]];
        std::vector<MapPoint *> want;
        int n = 0;
        if (!kb->isBad()) n = refbow::SearchByBoW(B.kfs[cur], kb, want, nnratio, ori);   // ref: src/LoopClosing.cc:318-324
        CHECK(vn[i] == n);
        CHECK(ids(vv[i]) == ids(want));
        g_matches += n;
        mix((unsigned long long)n);
        const std::vector<long> w = ids(want);
        for (size_t f = 0; f < w.size(); f++) mix((unsigned long long)(w[f] + 1) * 137u + f);
    }
}

// the same edits on both maps; what the class must hear of afterwards comes back through the lists (map A's objects)
struct Told {
    std::vector<MapPoint *> dead, flagged;
    std::vector<KeyFrame *> erasedKFs;
};

static void edit(World &A, World &B, int round, Told &T)
{
    World *Ws[2] = {&A, &B};
    for (int w = 0; w < 2; w++) {
        World &W = *Ws[w];
        g_seed = 700u + 41u * (unsigned)round;
        for (int e = 0; e < 30; e++) {                       // Replace: b takes a's observations
            MapPoint *a = W.pts[rnd(NPT)], *b = W.pts[rnd(NPT)];
            if (a == b || a->isBad() || b->isBad()) continue;
            a->Replace(b);
            if (w == 0) T.dead.push_back(a);
        }
        for (int e = 0; e < 60; e++) {                       // SetBadFlag of points: the rows keep naming them
            MapPoint *p = W.pts[rnd(NPT)];
            if (p->isBad()) continue;
            p->SetBadFlag();
            if (w == 0) T.flagged.push_back(p);
        }
        KeyFrame *gone = W.kfs[4 + 9 * round];               // an erased key frame (ref: KeyFrame::SetBadFlag's EraseObservation loop):
        for (int i = 0; i < gone->N; i++)                    // a bad candidate from now on
            if (gone->mvpMapPoints[i]) erase_observation(gone->mvpMapPoints[i], gone);
        gone->mbBad = true;
        if (w == 0) T.erasedKFs.push_back(gone);
        MapPoint *p = new_point(W);                          // a point that is never Put: its key frames go the host way
        for (int t = 0; t < 2; t++) {
            KeyFrame *kf = W.kfs[1 + 2 * round + 11 * t];
            for (int i = 0; i < kf->N; i++)
                if (!kf->mvpMapPoints[i]) { observe(p, kf, i); break; }
        }
    }
}

static void tell(Resident &R, World &A, Told &T)
{
    for (size_t i = 0; i < T.dead.size(); i++) R.LS.Erase(T.dead[i]), R.put.erase(T.dead[i]);
    for (size_t i = 0; i < T.flagged.size(); i++) R.LS.UpdateFlags(T.flagged[i]);
    for (size_t i = 0; i < T.erasedKFs.size(); i++) {
        R.LS.EraseKeyFrame(T.erasedKFs[i]);
        if (R.rows.size() > T.erasedKFs[i]->mnId) R.rows[T.erasedKFs[i]->mnId].clear();
    }
    R.sync(A);
    T = Told();
}

static std::vector<int> pick(unsigned seed, int n, bool twice)
{
    std::vector<int> v;
    g_seed = seed;
    for (int i = 0; i < n; i++) v.push_back((int)rnd(NKF));
    if (twice && n > 2) v[n - 1] = v[0];                     // a candidate twice
    return v;
}

int main()
{
    World A, B;
    build(A);
    build(B);
    Resident R;
    {
        std::vector<MapPoint *> all(A.pts.begin(), A.pts.begin() + NPT);
        R.LS.Put(all);
        R.put.insert(all.begin(), all.end());
    }
    for (int k = 0; k < NKF; k++)
        if (k % 5 != 2) R.put_kf(A.kfs[k]);                  // some key frames are left for the class to put
    std::vector<int> all;
    for (int k = 0; k < NKF; k++) all.push_back(k);

    reloc(R, A, B, all, 15, 0.75f, true, true);              // every key frame a candidate: the device way throughout
    CHECK(LocalMapSearch::BowCandCounts().device == NKF && LocalMapSearch::BowCandCounts().host == 0);
    R.sync(A);
    CHECK(g_matches > 100);
    reloc(R, A, B, pick(11, 7, true), 3, 0.75f, false, true);   // a low minMatches: segments of several candidates
    CHECK(g_setups > 20);
    reloc(R, A, B, pick(12, 5, false), 15, 0.9f, true, false);
    reloc(R, A, B, std::vector<int>(), 15, 0.75f, true, true);  // no candidate at all
    loop(R, A, B, 3, all, 0.75f, true);
    loop(R, A, B, 8, pick(13, 9, true), 0.75f, false);

    for (int round = 0; round < 3; round++) {
        Told T;
        edit(A, B, round, T);
        tell(R, A, T);
        reloc(R, A, B, all, 4, 0.75f, true, true);
        reloc(R, A, B, pick(20u + (unsigned)round, 6, true), 2, 0.75f, round != 1, true);
        loop(R, A, B, 5 + round, all, 0.75f, true);
        loop(R, A, B, 1 + 2 * round, pick(30u + (unsigned)round, 5, false), 0.75f, true);   // the current key frame goes the host way
        loop(R, A, B, 6, pick(40u + (unsigned)round, 4, false), 0.9f, false);
    }

    const long dev = LocalMapSearch::BowCandCounts().device, host = LocalMapSearch::BowCandCounts().host;
    CHECK(dev > 150 && host > 15);
    CHECK(g_matches > 1000 && g_setups > 200);
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %ld %ld %016llx\n", g_calls, dev, host, g_digest);
    return 0;
}
