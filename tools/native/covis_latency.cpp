// covis_latency.cpp -- what updating the covisibility graph of K key frames costs a C++ caller (tools/covis_latency.py; DESIGN.md
// section 20): a map of NKF key frames of NFEAT features, every point seen from about six key frames of a neighbourhood, the K
// key frames in the middle of the map updated back to back as LoopClosing::CorrectLoop does (K = 1: ProcessNewKeyFrame).
//   a_host    sequential KeyFrame::UpdateConnections of slamlite.h on the host objects: the baseline
//   b_call    orbhip_map_covis alone: counts, weights and orders of the K key frames, nothing applied
//   c_dropin  LocalMapSearch::UpdateConnections whole: the call, then AddConnection / the lists / the parent on the objects
// Before every timed call the graph members of every key frame are emptied (not timed), so a and c do the same per-neighbour
// AddConnection / UpdateBestCovisibles work.  The program fails unless a and c leave the same graph.  Prints
// "<mode> median <us> p10 <us> p90 <us>" per mode, "floor <us>" (orbhip_debug_roundtrip mode 1) and the shape.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "hiperror.h"
#include "orbhip.h"

using namespace ORB_SLAM2;
typedef std::chrono::steady_clock Clock;

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

struct Probe : LocalMapSearch {
    explicit Probe(int n) : LocalMapSearch(n) {}
    orbhip_ctx *ctx() { return mpCtx; }
};

static std::vector<KeyFrame *> g_kfs;
static std::vector<MapPoint *> g_pts;

static void build(int NKF, int NFEAT, int OBS, int WINDOW)
{
    g_seed = 2025;
    std::vector<int> nextFree(NKF, 0);
    for (int k = 0; k < NKF; k++) {
        KeyFrame *kf = new KeyFrame();
        kf->mnId = (long unsigned int)k;
        kf->N = NFEAT;
        kf->mvpMapPoints.assign(NFEAT, (MapPoint *)NULL);
        g_kfs.push_back(kf);
    }
    const int NPT = (int)((long)NKF * NFEAT / OBS);
    for (int j = 0; j < NPT; j++) {
        MapPoint *p = new MapPoint();
        p->mnId = (long unsigned int)j;
        p->mWorldPos = cv::Mat::zeros(3, 1, CV_32F), p->mNormalVector = cv::Mat::zeros(3, 1, CV_32F), p->mDescriptor = cv::Mat::zeros(1, 32, CV_8U);
        g_pts.push_back(p);
        const int n = std::max(1, OBS - 2 + (int)rnd(5)), centre = (int)rnd(NKF);
        for (int tries = 0; (int)p->mObservations.size() < n && tries < 100; tries++) {
            const int k = centre - WINDOW + (int)rnd(2 * WINDOW + 1);
            if (k < 0 || k >= NKF || p->IsInKeyFrame(g_kfs[k]) || nextFree[k] >= NFEAT) continue;
            const int idx = nextFree[k]++;
            g_kfs[k]->mvpMapPoints[idx] = p;
            p->AddObservation(g_kfs[k], idx);
        }
    }
}

static void reset_graph()
{
    for (size_t k = 0; k < g_kfs.size(); k++) {
        KeyFrame *kf = g_kfs[k];
        kf->mConnectedKeyFrameWeights.clear();
        kf->mvpOrderedConnectedKeyFrames.clear();
        kf->mvOrderedWeights.clear();
        kf->mspChildrens.clear();
        kf->mpParent = NULL;
        kf->mbFirstConnection = true;
    }
}

static unsigned long long digest(long *links)
{
    unsigned long long h = 1469598103934665603ull;
    *links = 0;
    for (size_t k = 0; k < g_kfs.size(); k++) {
        KeyFrame *kf = g_kfs[k];
        std::vector<std::pair<long unsigned int, int> > w;
        for (std::map<KeyFrame *, int>::iterator it = kf->mConnectedKeyFrameWeights.begin(); it != kf->mConnectedKeyFrameWeights.end(); ++it)
            w.push_back(std::make_pair(it->first->mnId, it->second));
        std::sort(w.begin(), w.end());
        for (size_t i = 0; i < w.size(); i++) h = (h ^ (((unsigned long long)w[i].first << 32) | (unsigned)w[i].second)) * 1099511628211ull;
        for (size_t i = 0; i < kf->mvpOrderedConnectedKeyFrames.size(); i++)
            h = (h ^ (((unsigned long long)kf->mvpOrderedConnectedKeyFrames[i]->mnId << 32) | (unsigned)kf->mvOrderedWeights[i])) * 1099511628211ull;
        h = (h ^ (kf->mpParent ? kf->mpParent->mnId + 1 : 0)) * 1099511628211ull;
        h = (h ^ kf->mspChildrens.size()) * 1099511628211ull;
        *links += (long)w.size();
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
    const int K = argc > 1 ? atoi(argv[1]) : 20, reps = argc > 2 ? atoi(argv[2]) : 30, NKF = argc > 3 ? atoi(argv[3]) : 200,
              NFEAT = argc > 4 ? atoi(argv[4]) : 1000;
    if (K < 1 || K > NKF || reps < 1 || NKF < 2 || NKF > 4096 || NFEAT < 1 || NFEAT > 8192)
        return printf("usage: covis_latency K reps [key frames <= 4096] [features <= 8192]\n"), 2;
    build(NKF, NFEAT, 6, 10);
    Probe LS((int)g_pts.size() + 64);
    if (!LS.ctx()) return printf("no device context: %s\n", OrbHipLastError()), 2;
    LS.InitKeyFrames(NKF, NFEAT);
    LS.Put(g_pts);
    for (int k = 0; k < NKF; k++) LS.PutKeyFrame(g_kfs[k]);
    std::vector<KeyFrame *> batch;
    std::vector<uint64_t> keys;
    for (int i = 0; i < K; i++) {
        KeyFrame *kf = g_kfs[(NKF - K) / 2 + i];
        batch.push_back(kf);
        keys.push_back((uint64_t)kf->mnId + 1);
    }
    const int cap = K * NKF;
    std::vector<int32_t> off(K + 1), nord(K), w(cap), order(cap);
    std::vector<uint64_t> nbr(cap);
    std::vector<double> t[3];
    unsigned long long want = 0;
    long links = 0;
    int total = 0;
    for (int r = -3; r < reps; r++) {
        for (int mode = 0; mode < 3; mode++) {
            reset_graph();
            const Clock::time_point t0 = Clock::now();
            if (mode == 0)
                for (int i = 0; i < K; i++) batch[i]->UpdateConnections();
            else if (mode == 1) {
                if (orbhip_map_covis(LS.ctx(), K, keys.data(), 15, off.data(), nbr.data(), w.data(), order.data(), nord.data(), cap, &total) != ORBHIP_OK)
                    return printf("orbhip_map_covis failed: %s\n", orbhip_last_error(LS.ctx())), 1;
            } else
                LS.UpdateConnections(batch);
            const double us = std::chrono::duration<double, std::micro>(Clock::now() - t0).count();
            if (r >= 0) t[mode].push_back(us);
            if (mode == 1) continue;
            const unsigned long long d = digest(&links);
            if (!want) want = d;
            if (d != want) return printf("mode %d: another graph\n", mode), 1;
        }
    }
    if (OrbHipErrorCount()) return printf("a drop-in call failed: %s\n", OrbHipLastError()), 1;
    if (LocalMapSearch::CovisCounts().host != 0) return printf("key frames went the host way: the measurement is not of the device call\n"), 1;
    const char *names[3] = {"a_host", "b_call", "c_dropin"};
    for (int m = 0; m < 3; m++) report(names[m], t[m]);
    double floorUs = 0;
    if (orbhip_debug_roundtrip(LS.ctx(), 1, 200, &floorUs) == ORBHIP_OK) printf("floor %.1f\n", floorUs);
    long nobs = 0;
    for (size_t i = 0; i < g_pts.size(); i++) nobs += (long)g_pts[i]->mObservations.size();
    printf("shape key_frames %d features %d points %d observations %ld queries %d links %d graph_links %ld\n", NKF, NFEAT, (int)g_pts.size(), nobs,
           K, total, links);
    for (size_t i = 0; i < g_pts.size(); i++) delete g_pts[i];
    for (size_t k = 0; k < g_kfs.size(); k++) delete g_kfs[k];
    return 0;
}
