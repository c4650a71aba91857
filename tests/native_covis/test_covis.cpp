// test_covis.cpp -- ORB_SLAM2::LocalMapSearch::UpdateConnections on mock KeyFrame / MapPoint objects: 40 key frames, 1500 points seen
// from 2 to 9 neighbouring key frames, three rounds of edits between updates -- Replace, SetBadFlag of points, an erased key frame,
// new key frames, a point that was never Put (its observers go the host way).  The map is built twice from one seed: the class
// works on one copy, sequential KeyFrame::UpdateConnections of slamlite.h on the other, and after every update
// mConnectedKeyFrameWeights, both ordered vectors, the parent and the children of every key frame are compared.  Every round updates
// once batched and once key frame by key frame; the last one also builds LoopConnections with an exclude list (ref:
// src/LoopClosing.cc:598-616).
//   -DCOVIS_MOCK  the class runs on the host model of the entry points (mock_covis.cc); no device, no liborbhip
//   otherwise     the class runs on liborbhip
// Prints "ok <updates> <key frames the device way> <key frames the host way> <digest>" and returns 0, or the failed checks.  The
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

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

static const int NKF = 40, NPT = 1500, NFEAT = 400, WINDOW = 7;

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

static KeyFrame *new_kf(World &W)
{
    KeyFrame *kf = new KeyFrame();
    kf->mnId = W.kfs.size();     // the same ids in both maps (the constructor counts across them)
    kf->N = NFEAT;
    kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
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

static void observe(World &W, MapPoint *p, int k)
{
    KeyFrame *kf = W.kfs[k];
    if (kf->isBad() || p->IsInKeyFrame(kf) || W.nextFree[k] >= kf->N) return;
    const int idx = W.nextFree[k]++;
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
}

// ref: src/MapPoint.cc EraseObservation, without the SetBadFlag of a point left with two observers
static void erase_observation(MapPoint *p, KeyFrame *kf)
{
    if (!p->mObservations.count(kf)) return;
    kf->mvpMapPoints[p->mObservations[kf]] = NULL;
    p->mObservations.erase(kf);
    p->nObs--;
}

static void build(World &W)
{
    g_seed = 4711;
    for (int k = 0; k < NKF; k++) new_kf(W);
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new_point(W);
        const int n = 2 + (int)rnd(8), centre = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 200; tries++) {
            const int k = centre - WINDOW + (int)rnd(2 * WINDOW + 1);
            if (k >= 0 && k < NKF) observe(W, p, k);
        }
    }
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }

static std::vector<long> ids(const std::vector<KeyFrame *> &v)
{
    std::vector<long> out;
    for (size_t i = 0; i < v.size(); i++) out.push_back((long)v[i]->mnId);
    return out;
}
static std::set<long> ids(const std::set<KeyFrame *> &s)
{
    std::set<long> out;
    for (std::set<KeyFrame *>::const_iterator it = s.begin(); it != s.end(); ++it) out.insert((long)(*it)->mnId);
    return out;
}
static std::map<long, int> ids(const std::map<KeyFrame *, int> &m)
{
    std::map<long, int> out;
    for (std::map<KeyFrame *, int>::const_iterator it = m.begin(); it != m.end(); ++it) out[(long)it->first->mnId] = it->second;
    return out;
}

// the graph members of every key frame of the two maps, by mnId
static void compare(World &A, World &B)
{
    bool weights = true, ordered = true, orderedW = true, tree = true;
    long links = 0;
    CHECK(A.kfs.size() == B.kfs.size());
    for (size_t i = 0; i < A.kfs.size() && i < B.kfs.size(); i++) {
        KeyFrame *a = A.kfs[i], *b = B.kfs[i];
        const std::map<long, int> wa = ids(a->mConnectedKeyFrameWeights);
        const std::vector<long> oa = ids(a->mvpOrderedConnectedKeyFrames);
        weights = weights && wa == ids(b->mConnectedKeyFrameWeights);
        ordered = ordered && oa == ids(b->mvpOrderedConnectedKeyFrames);
        orderedW = orderedW && a->mvOrderedWeights == b->mvOrderedWeights && a->mvOrderedWeights.size() == oa.size();
        const long pa = a->mpParent ? (long)a->mpParent->mnId : -1, pb = b->mpParent ? (long)b->mpParent->mnId : -1;
        tree = tree && pa == pb && ids(a->mspChildrens) == ids(b->mspChildrens) && a->mbFirstConnection == b->mbFirstConnection;
        for (std::map<long, int>::const_iterator it = wa.begin(); it != wa.end(); ++it) mix(((unsigned long long)it->first << 32) | (unsigned)it->second);
        for (size_t r = 0; r < oa.size(); r++) mix(((unsigned long long)oa[r] << 32) | (unsigned)a->mvOrderedWeights[r]);
        mix((unsigned long long)pa);
        links += (long)wa.size();
    }
    CHECK(weights);
    CHECK(ordered);
    CHECK(orderedW);
    CHECK(tree);
    CHECK(links > 300);
}

// ---- the class's side of the map: what the integrator tells LocalMapSearch ----
struct Resident {
    LocalMapSearch LS;
    std::set<MapPoint *> put;                          // the points the store knows
    std::vector<std::vector<MapPoint *> > rows;        // every key frame's row as the table has it (empty: no row)
    Resident() : LS(4096) { LS.InitKeyFrames(64, 512); }
    MapPoint *known(MapPoint *p) { return p && put.count(p) ? p : NULL; }
    void put_kf(KeyFrame *kf)
    {
        LS.PutKeyFrame(kf);
        noted(kf);
    }
    void noted(KeyFrame *kf)                           // (a row the class put by itself)
    {
        if (rows.size() <= kf->mnId) rows.resize(kf->mnId + 1);
        rows[kf->mnId].clear();
        for (int i = 0; i < kf->N; i++) rows[kf->mnId].push_back(known(kf->mvpMapPoints[i]));
    }
    // SetMapPoint for every entry that changed since the row was last in step
    void sync(World &A)
    {
        for (size_t k = 0; k < A.kfs.size() && k < rows.size(); k++) {
            KeyFrame *kf = A.kfs[k];
            if (rows[k].empty() || kf->isBad()) continue;
            for (int i = 0; i < kf->N; i++)
                if (known(kf->mvpMapPoints[i]) != rows[k][i]) {
                    rows[k][i] = known(kf->mvpMapPoints[i]);
                    LS.SetMapPoint(kf, (size_t)i, rows[k][i]);
                }
        }
    }
};

static int g_updates = 0;

static std::vector<int> live_order(World &W, unsigned seed)
{
    std::vector<int> v;
    for (size_t k = 0; k < W.kfs.size(); k++)
        if (!W.kfs[k]->isBad()) v.push_back((int)k);
    g_seed = seed;
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd((unsigned)i)]);
    return v;
}

static void update_batched(Resident &R, World &A, World &B, const std::vector<int> &which)
{
    std::vector<KeyFrame *> va;
    for (size_t i = 0; i < which.size(); i++) va.push_back(A.kfs[which[i]]), B.kfs[which[i]]->UpdateConnections();
    R.LS.UpdateConnections(va);
    for (size_t i = 0; i < va.size(); i++)
        if (R.rows.size() <= va[i]->mnId || R.rows[va[i]->mnId].empty()) R.noted(va[i]);
    g_updates++;
    compare(A, B);
}

static void update_singly(Resident &R, World &A, World &B, const std::vector<int> &which)
{
    for (size_t i = 0; i < which.size(); i++) {
        R.LS.UpdateConnections(A.kfs[which[i]]);
        B.kfs[which[i]]->UpdateConnections();
        g_updates++;
    }
    compare(A, B);
}

// the same edits on both maps; what the class must hear of afterwards comes back through the lists (map A's objects)
struct Told {
    std::vector<MapPoint *> dead, flagged;
    std::vector<KeyFrame *> erasedKFs, newKFs;
};

static void edit(World &A, World &B, int round, int phase, Told &T)
{
    World *Ws[2] = {&A, &B};
    for (int w = 0; w < 2; w++) {
        World &W = *Ws[w];
        g_seed = 900u + 37u * (unsigned)round + 5u * (unsigned)phase;
        for (int e = 0; e < 25; e++) {                      // Replace: b takes a's observations
            MapPoint *a = W.pts[rnd(NPT)], *b = W.pts[rnd(NPT)];
            if (a == b || a->isBad() || b->isBad()) continue;
            a->Replace(b);
            if (w == 0) T.dead.push_back(a);
        }
        for (int e = 0; e < 40; e++) {                      // SetBadFlag of points: the rows keep naming them
            MapPoint *p = W.pts[rnd(NPT)];
            if (p->isBad()) continue;
            p->SetBadFlag();
            if (w == 0) T.flagged.push_back(p);
        }
        if (phase == 0) {
            KeyFrame *gone = W.kfs[6 + 11 * round];          // an erased key frame (ref: KeyFrame::SetBadFlag's EraseObservation loop)
            for (int i = 0; i < gone->N; i++)
                if (gone->mvpMapPoints[i]) erase_observation(gone->mvpMapPoints[i], gone);
            gone->mbBad = true;
            if (w == 0) T.erasedKFs.push_back(gone);
            for (int nk = 0; nk < 2; nk++) {                 // new key frames over the points of a neighbourhood
                KeyFrame *kf = new_kf(W);
                const int k = (int)kf->mnId, centre = (int)rnd(NKF);
                for (int e = 0; e < 2500 && W.nextFree[k] < 160; e++) {
                    MapPoint *p = W.pts[rnd(NPT)];
                    if (p->isBad() || p->mObservations.empty()) continue;
                    bool near = false;
                    for (std::map<KeyFrame *, size_t>::iterator it = p->mObservations.begin(); it != p->mObservations.end(); ++it)
                        near = near || labs((long)it->first->mnId - centre) <= WINDOW;
                    if (near) observe(W, p, k);
                }
                if (w == 0) T.newKFs.push_back(kf);
            }
            MapPoint *p = new_point(W);                      // a point that is never Put: its observers go the host way
            observe(W, p, 2 + round), observe(W, p, 3 + round), observe(W, p, (int)W.kfs.size() - 2);
        }
    }
}

static void tell(Resident &R, World &A, Told &T, bool putLastNewKF)
{
    for (size_t i = 0; i < T.dead.size(); i++) R.LS.Erase(T.dead[i]), R.put.erase(T.dead[i]);
    for (size_t i = 0; i < T.flagged.size(); i++) R.LS.UpdateFlags(T.flagged[i]);
    for (size_t i = 0; i < T.erasedKFs.size(); i++) R.LS.EraseKeyFrame(T.erasedKFs[i]), R.rows[T.erasedKFs[i]->mnId].clear();
    for (size_t i = 0; i < T.newKFs.size(); i++)
        if (putLastNewKF || i + 1 < T.newKFs.size()) R.put_kf(T.newKFs[i]);
    R.sync(A);
    T = Told();
}

int main()
{
    World A, B;
    build(A);
    build(B);
    Resident R;
    R.LS.Put(A.pts);
    R.put.insert(A.pts.begin(), A.pts.end());
    for (int k = 0; k < NKF; k++)
        if (k != 17) R.put_kf(A.kfs[k]);                     // one key frame is left for the class to put
    update_batched(R, A, B, live_order(A, 1));
    CHECK(LocalMapSearch::CovisCounts().device == NKF && LocalMapSearch::CovisCounts().host == 0);
    {   // the rules bite in this scene: links below and above the threshold, a parent everywhere but at mnId 0
        long weak = 0, strong = 0;
        for (int k = 0; k < NKF; k++) {
            weak += A.kfs[k]->mConnectedKeyFrameWeights.size() > A.kfs[k]->mvOrderedWeights.size() ? 1 : 0;
            strong += (long)A.kfs[k]->mvOrderedWeights.size();
            CHECK((A.kfs[k]->mpParent != NULL) == (k != 0));
        }
        CHECK(strong > 100 && weak > 5);
    }
    update_singly(R, A, B, live_order(A, 2));                // nothing changed in between: the graph stays

    for (int round = 0; round < 3; round++) {
        Told T;
        edit(A, B, round, 0, T);
        tell(R, A, T, false);                                // the last new key frame gets its row from the batched update
        update_batched(R, A, B, live_order(A, 10u + (unsigned)round));
        edit(A, B, round, 1, T);
        tell(R, A, T, true);
        update_singly(R, A, B, live_order(A, 20u + (unsigned)round));
    }

    {   // CorrectLoop's second round over mvpCurrentConnectedKFs (ref: src/LoopClosing.cc:598-616) after one more set of edits
        Told T;
        edit(A, B, 3, 1, T);
        tell(R, A, T, true);
        std::vector<int> which = live_order(A, 33);
        which.resize(14);
        std::vector<KeyFrame *> va, vb;
        for (size_t i = 0; i < which.size(); i++) va.push_back(A.kfs[which[i]]), vb.push_back(B.kfs[which[i]]);
        std::map<KeyFrame *, std::set<KeyFrame *> > la, lb;
        for (size_t i = 0; i < vb.size(); i++) {
            KeyFrame *pKFi = vb[i];
            const std::vector<KeyFrame *> vpPreviousNeighbors = pKFi->GetVectorCovisibleKeyFrames();
            pKFi->UpdateConnections();
            std::set<KeyFrame *> &s = lb[pKFi];
            for (std::map<KeyFrame *, int>::iterator it = pKFi->mConnectedKeyFrameWeights.begin(); it != pKFi->mConnectedKeyFrameWeights.end(); ++it)
                s.insert(it->first);
            for (size_t j = 0; j < vpPreviousNeighbors.size(); j++) s.erase(vpPreviousNeighbors[j]);
            for (size_t j = 0; j < vb.size(); j++) s.erase(vb[j]);
        }
        R.LS.UpdateConnections(va, &la, &va);
        g_updates++;
        compare(A, B);
        CHECK(la.size() == lb.size());
        long fresh = 0;
        for (size_t i = 0; i < va.size(); i++) {
            const std::set<long> sa = ids(la[va[i]]);
            CHECK(sa == ids(lb[vb[i]]));
            fresh += (long)sa.size();
            for (std::set<long>::const_iterator it = sa.begin(); it != sa.end(); ++it) mix((unsigned long long)*it);
        }
        CHECK(fresh > 0);
    }

    const long dev = LocalMapSearch::CovisCounts().device, host = LocalMapSearch::CovisCounts().host;
    CHECK(dev > 100 && host > 10);
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %ld %ld %016llx\n", g_updates, dev, host, g_digest);
    return 0;
}
