// test_refresh.cpp -- ORB_SLAM2::LocalMapSearch::RefreshPoints on mock KeyFrame / MapPoint objects: 40 key frames, 1500 points seen
// from 2 to 9 of them (one from 36: more than the set limit of 32, so the host fallback runs beside the device call), three rounds
// of edits between refreshes -- added observations, erased observations, a Replace, a key frame turned bad, moved points.  The map
// is built twice from one seed: the class works on one copy, MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth of
// slamlite.h per point on the other, and after every refresh descriptors, normals and distance ranges are compared bit for bit,
// between the two maps and between the objects and the resident store (orbhip_map_get).
//   -DREFRESH_MOCK  the class runs on the host model of the entry points (mock_refresh.cc); no device, no liborbhip
//   otherwise       the class runs on liborbhip
// Prints "ok <refreshes> <points the device way> <points the host way> <digest>" and returns 0, or the failed checks.  The digest is
// over every refreshed value, so the two programs must print the same line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static float frand(float lo, float hi) { return lo + (hi - lo) * (float)rnd(1 << 16) / 65536.f; }

static const int NKF = 40, NPT = 1500, NFEAT = 420, NLEVELS = 8, SET_LIMIT = 32, MANY = 36;

struct Probe : LocalMapSearch {   // the store behind the class, for the read-back
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

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

// the point seen from a free feature of key frame k.  While the map is built (base != NULL) the feature's descriptor becomes the
// point's own with a few bits flipped; afterwards the feature keeps the descriptor it has: a key frame's features never change once
// it exists, which is what lets them stay resident
static void observe(World &W, MapPoint *p, int k, const uint8_t *base)
{
    KeyFrame *kf = W.kfs[k];
    if (p->IsInKeyFrame(kf) || W.nextFree[k] >= kf->N) return;
    const int idx = W.nextFree[k]++;
    if (base) {
        uint8_t *d = kf->mDescriptors.ptr(idx);
        memcpy(d, base, 32);
        for (unsigned b = rnd(5); b > 0; b--) d[rnd(32)] ^= (uint8_t)(1u << rnd(8));
    }
    kf->mvpMapPoints[idx] = p;
    p->AddObservation(kf, idx);
    if (!p->mpRefKF) p->mpRefKF = kf;
}

// ref: src/MapPoint.cc EraseObservation, without the SetBadFlag of a point left with two observers
static void erase_observation(MapPoint *p, KeyFrame *kf)
{
    if (!p->mObservations.count(kf)) return;
    kf->mvpMapPoints[p->mObservations[kf]] = NULL;
    p->mObservations.erase(kf);
    p->nObs--;
    if (p->mpRefKF == kf) {
        p->mpRefKF = NULL;
        for (std::map<KeyFrame *, size_t>::iterator it = p->mObservations.begin(); it != p->mObservations.end(); ++it)
            if (!p->mpRefKF || it->first->mnId < p->mpRefKF->mnId) p->mpRefKF = it->first;
    }
}

static void build(World &W)
{
    g_seed = 90210;
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        W.kfs.push_back(kf);
        kf->N = NFEAT;
        kf->Ow = cv::Mat(3, 1, CV_32F);
        for (int c = 0; c < 3; c++) kf->Ow.at<float>(c, 0) = frand(-3.f, 3.f);
        kf->Tcw = cv::Mat::zeros(4, 4, CV_32F);
        kf->mnMinX = 0, kf->mnMaxX = 640, kf->mnMinY = 0, kf->mnMaxY = 480;
        kf->mfGridElementWidthInv = 64.f / 640.f, kf->mfGridElementHeightInv = 48.f / 480.f;
        kf->mnScaleLevels = NLEVELS, kf->mfScaleFactor = 1.2f, kf->mfLogScaleFactor = logf(1.2f);
        float s = 1.f;
        for (int l = 0; l < NLEVELS; l++, s *= 1.2f) {
            kf->mvScaleFactors.push_back(s);
            kf->mvLevelSigma2.push_back(s * s);
            kf->mvInvLevelSigma2.push_back(1.f / (s * s));
        }
        kf->mDescriptors = cv::Mat(NFEAT, 32, CV_8U);
        for (int i = 0; i < NFEAT; i++) {
            kf->mvKeys.push_back(cv::KeyPoint(frand(2, 637), frand(2, 477), 31.f, frand(0, 360), 20.f, (int)rnd(NLEVELS), -1));
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
        for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c, 0) = frand(-6.f, 6.f) + (c == 2 ? 9.f : 0.f), p->mNormalVector.at<float>(c, 0) = 0.f;
        for (int b = 0; b < 32; b++) p->mDescriptor.ptr(0)[b] = (uint8_t)rnd(256);
        p->mfMaxDistance = 12.f, p->mfMinDistance = 3.f;
        uint8_t base[32];
        memcpy(base, p->mDescriptor.ptr(0), 32);
        // most points live among the first 32 key frames; every fifth may be seen from the last eight as well
        const int n = j == 7 ? MANY : 2 + (int)rnd(8), span = j == 7 ? NKF : (j % 5 == 0 ? NKF : SET_LIMIT);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 400; tries++) observe(W, p, (int)rnd(span), base);
    }
}

static unsigned long long g_digest = 1469598103934665603ull;
static void mix(unsigned long long v) { g_digest = (g_digest ^ v) * 1099511628211ull; }
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

// descriptors, normals and ranges of the two maps, and of the store behind the class, bit for bit
static void compare(Probe &LS, World &A, World &B)
{
    bool desc = true, geo = true, store = true;
    std::vector<uint64_t> keys;
    std::vector<MapPoint *> live;
    for (size_t i = 0; i < A.pts.size(); i++) {
        MapPoint *a = A.pts[i], *b = B.pts[i];
        desc = desc && memcmp(a->mDescriptor.ptr(0), b->mDescriptor.ptr(0), 32) == 0;
        for (int c = 0; c < 3; c++) {
            geo = geo && bits(a->mNormalVector.at<float>(c, 0)) == bits(b->mNormalVector.at<float>(c, 0));
            mix(bits(a->mNormalVector.at<float>(c, 0)));
        }
        geo = geo && bits(a->mfMinDistance) == bits(b->mfMinDistance) && bits(a->mfMaxDistance) == bits(b->mfMaxDistance);
        mix(((unsigned long long)bits(a->mfMinDistance) << 32) | bits(a->mfMaxDistance));
        for (int w = 0; w < 4; w++) {
            unsigned long long v;
            memcpy(&v, a->mDescriptor.ptr(0) + 8 * w, 8);
            mix(v);
        }
        if (!a->isBad()) keys.push_back((uint64_t)a->mnId + 1), live.push_back(a);
    }
    CHECK(desc);
    CHECK(geo);
    const size_t n = keys.size();
    std::vector<float> nrm(3 * n), mn(n), mx(n);
    std::vector<uint8_t> d(32 * n);
    CHECK(orbhip_map_get(LS.ctx(), (int)n, keys.data(), NULL, nrm.data(), mn.data(), mx.data(), d.data(), NULL) == ORBHIP_OK);
    for (size_t i = 0; i < n; i++) {
        MapPoint *a = live[i];
        store = store && memcmp(a->mDescriptor.ptr(0), &d[32 * i], 32) == 0 && bits(a->mfMinDistance) == bits(mn[i]) &&
                bits(a->mfMaxDistance) == bits(mx[i]);
        for (int c = 0; c < 3; c++) store = store && bits(a->mNormalVector.at<float>(c, 0)) == bits(nrm[3 * i + c]);
    }
    CHECK(store);
}

static int g_refreshes = 0;

// the class on A, the per-point methods on B (ref: src/LocalMapping.cc:2577-2590: descriptor, then normal and depth)
static void refresh(Probe &LS, World &A, World &B, const std::vector<int> &which, bool bDesc = true, bool bNormals = true)
{
    std::vector<MapPoint *> va;
    int want = 0;
    std::vector<char> once(A.pts.size(), 0);
    for (size_t i = 0; i < which.size(); i++) {
        if (which[i] < 0) { va.push_back(NULL); continue; }
        va.push_back(A.pts[which[i]]);
        MapPoint *b = B.pts[which[i]];
        if (b->isBad() || once[which[i]]) continue;
        once[which[i]] = 1;
        if (b->mObservations.empty()) continue;
        if (bDesc) b->ComputeDistinctiveDescriptors();
        if (bNormals) b->UpdateNormalAndDepth();
        want++;
    }
    CHECK(LS.RefreshPoints(va, bDesc, bNormals) == want);
    g_refreshes++;
    compare(LS, A, B);
}

int main()
{
    World A, B;
    build(A);
    build(B);
    Probe LS(4096);
    CHECK(LS.SetLimit(SET_LIMIT) == SET_LIMIT);          // fewer sets than key frames: points seen from the last eight go the host way
    LS.Put(A.pts);
    std::vector<int> all, some;
    for (int j = 0; j < NPT; j++) all.push_back(j);
    refresh(LS, A, B, all);
    const long dev0 = LocalMapSearch::RefreshCounts().device, host0 = LocalMapSearch::RefreshCounts().host;
    printf("# first refresh: %ld points the device way, %ld the host way\n", dev0, host0);
    CHECK(dev0 >= 1000 && host0 >= 100 && dev0 + host0 == NPT);

    for (int round = 0; round < 3; round++) {
        World *Ws[2] = {&A, &B};
        const unsigned seed = 777u + 31u * (unsigned)round;
        std::vector<MapPoint *> moved, dead;
        for (int w = 0; w < 2; w++) {                     // the same edits on both maps
            World &W = *Ws[w];
            g_seed = seed;
            for (int e = 0; e < 120; e++) {               // added observations
                MapPoint *p = W.pts[rnd(NPT)];
                const int k = (int)rnd(SET_LIMIT + 2 * round);
                if (!p->isBad()) observe(W, p, k, NULL);
            }
            for (int e = 0; e < 120; e++) {               // erased observations (never the last one)
                MapPoint *p = W.pts[rnd(NPT)];
                if (p->isBad() || p->mObservations.size() < 2) continue;
                std::map<KeyFrame *, size_t>::iterator it = p->mObservations.begin();
                KeyFrame *kf = it->first;                  // the lowest mnId among them: the same key frame in both maps
                for (; it != p->mObservations.end(); ++it)
                    if (it->first->mnId < kf->mnId) kf = it->first;
                erase_observation(p, kf);
            }
            const int a = 20 + 50 * round, b = a + 1;     // a Replace: b takes a's observations
            if (!W.pts[a]->isBad() && !W.pts[b]->isBad()) {
                W.pts[a]->Replace(W.pts[b]);
                if (w == 0) dead.push_back(W.pts[a]);
            }
            W.kfs[3 + 9 * round]->mbBad = true;            // a key frame turned bad (its points still name it)
            for (int e = 0; e < 200; e++) {               // points moved by a bundle adjustment
                MapPoint *p = W.pts[rnd(NPT)];
                for (int c = 0; c < 3; c++) p->mWorldPos.at<float>(c, 0) += frand(-0.05f, 0.05f);
                if (w == 0 && !p->isBad()) moved.push_back(p);
            }
        }
        for (size_t i = 0; i < dead.size(); i++) LS.Erase(dead[i]);   // what the integrator does after Replace ...
        for (size_t i = 1; i < moved.size(); i++)                      // ... and after SetWorldPos (each point once)
            for (size_t j = 0; j < i; j++)
                if (moved[j] == moved[i]) { moved.erase(moved.begin() + i), i--; break; }
        LS.Put(moved);
        if (round == 1) {                                  // after a bundle adjustment: UpdateNormalAndDepth alone, then the rest
            refresh(LS, A, B, all, false, true);
            refresh(LS, A, B, all, true, false);
        } else {
            some.clear();                                  // a key frame's points, with NULLs and second occurrences, then everything
            KeyFrame *kf = A.kfs[5 + round];
            for (int i = 0; i < kf->N; i++) {
                MapPoint *p = kf->mvpMapPoints[i];
                some.push_back(p ? (int)(p->mnId - A.pts[0]->mnId) : -1);
                if (p && i % 7 == 0) some.push_back(some.back());
            }
            refresh(LS, A, B, some);
            refresh(LS, A, B, all);
        }
    }
    const long dev = LocalMapSearch::RefreshCounts().device, host = LocalMapSearch::RefreshCounts().host;
    CHECK(OrbHipErrorCount() == 0);
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %ld %ld %016llx\n", g_refreshes, dev, host, g_digest);
    return 0;
}
