// bowcand_latency.cpp -- what SearchByBoW against K candidate key frames costs a C++ caller (tools/bowcand_latency.py; DESIGN.md
// section 21): one frame (mode 0, Tracking::Relocalization) or key frame (mode 1, LoopClosing::ComputeSim3) of NFEAT features against
// K resident candidates of NFEAT features each, 100 vocabulary nodes (a k = 10 / L = 6 vocabulary at levelsup 4), the candidates'
// descriptors noisy copies of the fixed side's so that the loops have matches to make; six of ten features hold a point.
//   a_host    K calls of ORBmatcher::SearchByBoW, in mode 0 each followed by the PnPsolver-constructor loop on the host: the baseline
//   b_call    orbhip_search_by_bow_candidates alone (mode 0: with the PnP arrays)
//   c_dropin  LocalMapSearch::SearchByBoWCandidates whole: the checks, the call, indices back to MapPoint*, the setups
//   d_oracle  the reference loops of tests/native_bowcand/ref_bowcand.h on one host core
// The program fails unless a, c and d give the same matches.  Prints "<mode> median <us> p10 <us> p90 <us>" per mode, "floor <us>"
// (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "ORBmatcher.h"
#include "hiperror.h"
#include "orbhip.h"
#include "ref_bowcand.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static const int NNODES = 100, NLEVELS = 8;
static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;

static void base_features(int n, std::vector<cv::KeyPoint> &keys, cv::Mat &desc, std::vector<int> &node)
{
    keys.resize(n), node.resize(n);
    desc = cv::Mat::zeros(n, 32, CV_8U);
    for (int i = 0; i < n; i++) {
        keys[i].pt.x = (float)rnd(640) + 0.25f, keys[i].pt.y = (float)rnd(480) + 0.5f;
        keys[i].angle = (float)rnd(360), keys[i].octave = (int)rnd(NLEVELS);
        for (int b = 0; b < 32; b++) desc.ptr(i)[b] = (unsigned char)rnd(256);
        node[i] = (int)rnd(NNODES);
    }
}

static void fv_of(const std::vector<int> &node, DBoW2::FeatureVector &fv)
{
    fv.clear();
    for (size_t i = 0; i < node.size(); i++) fv[(unsigned)node[i]].push_back((unsigned)i);
}

// a key frame that sees the base scene: a shuffled copy with ~12 flipped bits per descriptor and a small turn
static KeyFrame *noisy_kf(int id, const std::vector<cv::KeyPoint> &keys, const cv::Mat &desc, const std::vector<int> &node)
{
    const int n = (int)keys.size();
    KeyFrame *kf = new KeyFrame();
    kf->mnId = (long unsigned int)id;
    kf->N = n;
    kf->mvKeysUn.resize(n);
    kf->mDescriptors = cv::Mat::zeros(n, 32, CV_8U);
    std::vector<int> nd(n);
    const int shift = (int)rnd((unsigned)n);
    for (int i = 0; i < n; i++) {
        const int s = (i + shift) % n;
        kf->mvKeysUn[i] = keys[s];
        kf->mvKeysUn[i].angle = keys[s].angle + (float)rnd(8);
        memcpy(kf->mDescriptors.ptr(i), desc.ptr(s), 32);
        for (int f = 0; f < 12; f++) kf->mDescriptors.ptr(i)[rnd(32)] ^= (unsigned char)(1u << rnd(8));
        nd[i] = rnd(10) ? node[s] : (int)rnd(NNODES);      // one in ten falls under another node
    }
    kf->mvKeys = kf->mvKeysUn;
    fv_of(nd, kf->mFeatVec);
    kf->mvpMapPoints.assign(n, (MapPoint *)NULL);
    for (int i = 0; i < n; i++) {
        if (rnd(10) >= 6) continue;
        MapPoint *p = new MapPoint();
        p->mnId = (long unsigned int)g_pts.size();
        p->mWorldPos = cv::Mat::zeros(3, 1, CV_32F), p->mNormalVector = cv::Mat::zeros(3, 1, CV_32F), p->mDescriptor = cv::Mat::zeros(1, 32, CV_8U);
        for (int r = 0; r < 3; r++) p->mWorldPos.at<float>(r, 0) = (float)rnd(2000) * 0.01f;
        g_pts.push_back(p);
        kf->mvpMapPoints[i] = p;
        p->AddObservation(kf, i);
    }
    return kf;
}

static unsigned long long digest(const std::vector<std::vector<MapPoint *> > &vv, const std::vector<int> &vn, long *matches)
{
    unsigned long long h = 1469598103934665603ull;
    *matches = 0;
    for (size_t k = 0; k < vv.size(); k++) {
        h = (h ^ (unsigned long long)vn[k]) * 1099511628211ull;
        *matches += vn[k];
        for (size_t i = 0; i < vv[k].size(); i++) h = (h ^ (vv[k][i] ? vv[k][i]->mnId + 1 : 0)) * 1099511628211ull;
    }
    return h;
}

static void report(const char *name, std::vector<double> &t)
{
    std::sort(t.begin(), t.end());
    const size_t m = t.size();
    printf("%s median %.1f p10 %.1f p90 %.1f\n", name, t[m / 2], t[m / 10], t[m - 1 - m / 10]);
}

int main(int argc, char **argv)
{
    const int mode = argc > 1 ? atoi(argv[1]) : 0, K = argc > 2 ? atoi(argv[2]) : 10, reps = argc > 3 ? atoi(argv[3]) : 30,
              NFEAT = argc > 4 ? atoi(argv[4]) : 1000;
    if ((mode != 0 && mode != 1) || K < 1 || K > 90 || reps < 1 || NFEAT < 16 || NFEAT > 8192)
        return printf("usage: bowcand_latency mode(0|1) K(<= 90) reps [features <= 8192]\n"), 2;
    g_seed = 31337;
    std::vector<cv::KeyPoint> keys;
    cv::Mat desc;
    std::vector<int> node;
    base_features(NFEAT, keys, desc, node);
    Frame F;
    F.mnId = 70000, F.N = NFEAT, F.mvKeysUn = keys, F.mvKeys = keys, F.mDescriptors = desc, F.mnScaleLevels = NLEVELS;
    fv_of(node, F.mFeatVec);
    F.mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
    float s = 1.f;
    for (int l = 0; l < NLEVELS; l++, s *= 1.2f) F.mvScaleFactors.push_back(s), F.mvLevelSigma2.push_back(s * s);
    for (int k = 0; k <= K; k++) g_kfs.push_back(noisy_kf(k, keys, desc, node));
    KeyFrame *cur = g_kfs[K];                                // mode 1: the current key frame
    std::vector<KeyFrame *> cands(g_kfs.begin(), g_kfs.begin() + K);

    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(K + 8, NFEAT);
    LS.Put(g_pts);
    for (size_t k = 0; k < g_kfs.size(); k++) LS.PutKeyFrame(g_kfs[k]);

    std::vector<std::vector<MapPoint *> > vv(K);
    std::vector<int> vn(K);
    std::vector<RelocCorrespondences> vs(K);
    // what b_call needs: the keys the drop-in uses (the sets are resident after the first c_dropin call)
    std::vector<orbhip_bow_candidate> cd(K);
    for (int k = 0; k < K; k++) cd[k].set_key = (1ull << 62) | (uint64_t)(k + 1), cd[k].row_key = (uint64_t)(k + 1);
    const uint64_t fixedSet = mode == 0 ? (uint64_t)F.mnId + 1 : ((1ull << 62) | (uint64_t)(K + 1));
    const int cap = K * NFEAT;
    std::vector<int32_t> matches((size_t)cap), nm(K), off(K + 1), kp(cap), kf(cap);
    std::vector<float> P3((size_t)cap * 3), P2((size_t)cap * 2), me(cap);
    int total = 0;

    std::vector<double> t[4];
    unsigned long long want = 0;
    long nmatch = 0, ncorr = 0;
    const int order[4] = {2, 0, 1, 3};                       // the drop-in first: it puts the sets b_call names
    for (int r = -3; r < reps; r++) {
        for (int o = 0; o < 4; o++) {
            const int m = order[o];
            const Clock::time_point t0 = Clock::now();
            if (m == 0) {
                ORBmatcher matcher(0.75f, true);
                for (int k = 0; k < K; k++) {
                    vn[k] = mode == 0 ? matcher.SearchByBoW(cands[k], F, vv[k]) : matcher.SearchByBoW(cur, cands[k], vv[k]);
                    if (mode == 0 && vn[k] >= 15) refbow::PnPSetup(F, vv[k], 5.991f, vs[k]);
                }
            } else if (m == 1) {
                const int rc = mode == 0 ? orbhip_search_by_bow_candidates(LS.ctx(), 0, fixedSet, 0, cd.data(), K, 50, 0.75f, 1, matches.data(), nm.data(), 15,
                                                                           F.mvLevelSigma2.data(), NLEVELS, 5.991f, off.data(), kp.data(), kf.data(), P3.data(),
                                                                           P2.data(), me.data(), cap, &total)
                                         : orbhip_search_by_bow_candidates(LS.ctx(), 1, fixedSet, (uint64_t)(K + 1), cd.data(), K, 50, 0.75f, 1, matches.data(),
                                                                           nm.data(), 0, NULL, 0, 0.f, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL);
                if (rc != ORBHIP_OK) return printf("orbhip_search_by_bow_candidates failed: %s\n", orbhip_last_error(LS.ctx())), 1;
            } else if (m == 2) {
                if (mode == 0) LS.SearchByBoWCandidates(cands, F, vv, vn, &vs, 15, 5.991f, 0.75f, true);
                else LS.SearchByBoWCandidates(cur, cands, vv, vn, 0.75f, true);
            } else {
                for (int k = 0; k < K; k++) {
                    vn[k] = mode == 0 ? refbow::SearchByBoW(cands[k], F, vv[k], 0.75f, true) : refbow::SearchByBoW(cur, cands[k], vv[k], 0.75f, true);
                    if (mode == 0 && vn[k] >= 15) refbow::PnPSetup(F, vv[k], 5.991f, vs[k]);
                }
            }
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[m].push_back(us);
            if (m == 1) continue;
            const unsigned long long d = digest(vv, vn, &nmatch);
            if (!want) want = d;
            if (d != want) return printf("mode %d: other matches\n", m), 1;
            if (mode == 0) {
                ncorr = 0;
                for (int k = 0; k < K; k++) ncorr += vn[k] >= 15 ? (long)vs[k].mvP2D.size() : 0;
            }
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    if (LocalMapSearch::BowCandCounts().host != 0) return printf("candidates went the host way: the measurement is not of the device call\n"), 1;
    const char *names[4] = {"a_host", "b_call", "c_dropin", "d_oracle"};
    for (int m = 0; m < 4; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    printf("shape mode %d candidates %d features %d nodes %d points %d matches %ld correspondences %ld\n", mode, K, NFEAT, NNODES, (int)g_pts.size(),
           nmatch, ncorr);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
