// tri_latency.cpp -- SearchForTriangulation of one key frame of 1000 features against K neighbours, from a C++ caller of the C ABI
// (tools/tri_latency.py runs it and writes profiles/triangulation/first_measurement.md).  In one process, on the same inputs,
// with the results compared for equality first:
//   (a) K orbhip_search_for_triangulation calls: everything travels with every call;
//   (b) one orbhip_search_for_triangulation_sets call, the K + 1 sets resident;
//   (c) the same with the sets put cold: orbhip_set_drop(all), K + 1 orbhip_set_put, the call;
//   (d) the oracle's orbo_search_for_triangulation K times on one host core (liborb_oracle.so, path in argv[1]).
// Prints one line: TRI_JSON {...} with the median microseconds of each for K = 10 and K = 20.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "orbhip.h"
#include "tri_scene.h"

typedef int (*oracle_fn)(const void *, const uint8_t *, int, const uint8_t *, const float *, const int32_t *, const int32_t *,
                         const int32_t *, int, const void *, const uint8_t *, int, const uint8_t *, const float *, const int32_t *,
                         const int32_t *, const int32_t *, int, const float *, float, float, const float *, const float *, int, int, int,
                         int32_t *);

struct Flat {
    int n;
    std::vector<uint8_t> desc, skip;
    std::vector<int32_t> node, off, idx;
    const orbhip_keypoint *kps;
    const float *ur;
    explicit Flat(ORB_SLAM2::KeyFrame *k) : n(k->N), desc((size_t)k->N * 32), skip(k->N)
    {
        for (int i = 0; i < n; i++) {
            memcpy(&desc[(size_t)i * 32], k->mDescriptors.ptr(i), 32);
            skip[i] = k->mvpMapPoints[i] ? 1 : 0;
        }
        off.push_back(0);
        for (DBoW2::FeatureVector::const_iterator it = k->mFeatVec.begin(); it != k->mFeatVec.end(); ++it) {
            node.push_back((int32_t)it->first);
            for (size_t j = 0; j < it->second.size(); j++) idx.push_back((int32_t)it->second[j]);
            off.push_back((int32_t)idx.size());
        }
        kps = reinterpret_cast<const orbhip_keypoint *>(k->mvKeysUn.data());
        ur = k->mvuRight.data();
    }
};

template <class F>
static double median_us(F fn, int warm, int n)
{
    for (int i = 0; i < warm; i++) fn();
    std::vector<double> t(n);
    for (int i = 0; i < n; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        t[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::sort(t.begin(), t.end());
    return 0.5 * (t[(n - 1) / 2] + t[n / 2]);
}

#define MUST(expr)                                                                                        \
    do {                                                                                                  \
        if ((expr) != ORBHIP_OK) { fprintf(stderr, "%s: %s\n", #expr, orbhip_last_error(ctx)); exit(1); } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s path/to/liborb_oracle.so [calls]\n", argv[0]); return 2; }
    const int calls = argc > 2 ? atoi(argv[2]) : 300;
    void *lib = dlopen(argv[1], RTLD_NOW);
    oracle_fn oracle = lib ? (oracle_fn)dlsym(lib, "orbo_search_for_triangulation") : NULL;
    if (!oracle) { fprintf(stderr, "cannot load the oracle from %s\n", argv[1]); return 2; }
    orbhip_ctx *ctx = orbhip_create(0, 50, 1.2f, 1, 20, 7, 128, 128, 1);
    if (!ctx) { fprintf(stderr, "no context: %s\n", orbhip_last_error(NULL)); return 1; }
    std::string json = "{";
    const int Ks[2] = {10, 20};
    for (int q = 0; q < 2; q++) {
        const int K = Ks[q], NF = 1000;
        tri::Scene S;
        // every key frame 1000 features (make_scene varies the sizes: ask for more and cut), stereo with ~60 % right coordinates
        tri::make_scene(S, K, NF + 17 * 3 + K, 5 + K, [](int) { return 1; }, 100);   // ~100 shared nodes of ~10 features, as at levelsup 4
        for (int k = 0; k <= K; k++) {
            ORB_SLAM2::KeyFrame &kf = S.kf[k];
            DBoW2::FeatureVector fv;
            for (DBoW2::FeatureVector::const_iterator it = kf.mFeatVec.begin(); it != kf.mFeatVec.end(); ++it)
                for (size_t j = 0; j < it->second.size(); j++)
                    if ((int)it->second[j] < NF) fv.addFeature(it->first, it->second[j]);
            kf.mFeatVec = fv;
            kf.N = NF;
            kf.mvKeysUn.resize(NF);
            kf.mvpMapPoints.resize(NF);
            kf.mvuRight.resize(NF);
        }
        std::vector<Flat> F;
        for (int k = 0; k <= K; k++) F.push_back(Flat(&S.kf[k]));
        const std::vector<float> &sf = S.kf[1].mvScaleFactors, &sg = S.kf[1].mvLevelSigma2;
        std::vector<orbhip_tri_neighbour> nb(K);
        std::vector<uint8_t> skip2;
        std::vector<float> ur2;
        for (int k = 0; k < K; k++) {
            nb[k].key2 = 2 + k;
            for (int i = 0; i < 9; i++) nb[k].F12[i] = S.F12[k].at<float>(i / 3, i % 3);
            nb[k].ex = 900.f + 10.f * k;      // far from every feature; the epipole's arithmetic is the host's either way
            nb[k].ey = 700.f;
            skip2.insert(skip2.end(), F[k + 1].skip.begin(), F[k + 1].skip.end());
            ur2.insert(ur2.end(), F[k + 1].ur, F[k + 1].ur + NF);
        }
        std::vector<int32_t> mA((size_t)K * NF), mB((size_t)K * NF), mD((size_t)K * NF), nB(K);
        std::vector<int> nA(K), nD(K);
        auto single = [&]() {
            for (int k = 0; k < K; k++)
                MUST(orbhip_search_for_triangulation(ctx, F[0].kps, F[0].desc.data(), NF, F[0].skip.data(), F[0].ur, F[0].node.data(),
                                                     F[0].off.data(), F[0].idx.data(), (int)F[0].node.size(), F[k + 1].kps, F[k + 1].desc.data(), NF,
                                                     F[k + 1].skip.data(), F[k + 1].ur, F[k + 1].node.data(), F[k + 1].off.data(),
                                                     F[k + 1].idx.data(), (int)F[k + 1].node.size(), nb[k].F12, nb[k].ex, nb[k].ey, sf.data(), sg.data(),
                                                     (int)sf.size(), 0, 0, &mA[(size_t)k * NF], &nA[k]));
        };
        auto put_all = [&]() {
            for (int k = 0; k <= K; k++)
                MUST(orbhip_set_put(ctx, 1 + k, F[k].kps, F[k].desc.data(), NF, F[k].node.data(), F[k].off.data(), F[k].idx.data(),
                                    (int)F[k].node.size(), 0.f, 0.f, 64.f / 640.f, 48.f / 480.f));
        };
        auto batched = [&]() {
            MUST(orbhip_search_for_triangulation_sets(ctx, 1, F[0].skip.data(), F[0].ur, nb.data(), K, skip2.data(), ur2.data(), sf.data(),
                                                      sg.data(), (int)sf.size(), 0, 0, mB.data(), nB.data()));
        };
        auto cold = [&]() {
            MUST(orbhip_set_drop(ctx, 0));
            put_all();
            batched();
        };
        auto host = [&]() {
            for (int k = 0; k < K; k++)
                nD[k] = oracle(F[0].kps, F[0].desc.data(), NF, F[0].skip.data(), F[0].ur, F[0].node.data(), F[0].off.data(), F[0].idx.data(),
                               (int)F[0].node.size(), F[k + 1].kps, F[k + 1].desc.data(), NF, F[k + 1].skip.data(), F[k + 1].ur,
                               F[k + 1].node.data(), F[k + 1].off.data(), F[k + 1].idx.data(), (int)F[k + 1].node.size(), nb[k].F12, nb[k].ex,
                               nb[k].ey, sf.data(), sg.data(), 0, 0, 50, &mD[(size_t)k * NF]);
        };
        // equality first
        single();
        put_all();
        batched();
        host();
        long total = 0;
        for (int k = 0; k < K; k++) {
            if (nA[k] != nB[k] || nA[k] != nD[k]) { fprintf(stderr, "K = %d, neighbour %d: %d / %d / %d matches\n", K, k, nA[k], nB[k], nD[k]); return 1; }
            total += nA[k];
        }
        if (mA != mB || mA != mD) { fprintf(stderr, "K = %d: the match rows differ\n", K); return 1; }
        if (total < 20L * K) { fprintf(stderr, "K = %d: only %ld matches, not a workload\n", K, total); return 1; }
        const double a = median_us(single, 20, calls), b = median_us(batched, 20, calls), c = median_us(cold, 5, std::max(10, calls / 10)),
                     d = median_us(host, 3, std::max(10, calls / 10));
        char buf[256];
        snprintf(buf, sizeof buf, "%s\"K%d\": {\"single_us\": %.2f, \"batched_us\": %.2f, \"cold_us\": %.2f, \"oracle_us\": %.2f, \"matches\": %ld}",
                 q ? ", " : "", K, a, b, c, d, total);
        json += buf;
        MUST(orbhip_set_drop(ctx, 0));
    }
    printf("TRI_JSON %s}\n", json.c_str());
    orbhip_destroy(ctx);
    return 0;
}
