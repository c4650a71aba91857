// test_trisearch_mock.cpp -- ORB_SLAM2::TriangulationSearch against a host model of orbhip_search_for_triangulation_sets and of
// the orbhip_set_* calls it uses (mock_trisearch.cc): no device.  What the class itself decides is checked: which key frames
// it puts and when it puts them again (set identity), the limit it asks for, the order in which the neighbours' flags are
// concatenated, the epipoles, and the order of the pairs.  The expectation per neighbour is the reference's
// SearchForTriangulation restated on the key frame's own data (tri::flat_search) with the epipole restated here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "TriangulationSearch.h"
#include "hiperror.h"
#include "mock_trisearch.h"
#include "tri_scene.h"

using namespace ORB_SLAM2;
typedef std::vector<std::pair<size_t, size_t> > Pairs;

static int g_checks = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checks++;                                                                      \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// ref: src/ORBmatcher.cc:664-671 with the gemm of R2w*Cw+t2w accumulated in double and rounded once
static void epipole(KeyFrame *k1, KeyFrame *k2, float &ex, float &ey)
{
    float C2[3];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int c = 0; c < 3; c++) s += (double)k2->Tcw.at<float>(r, c) * (double)k1->Ow.at<float>(c, 0);
        C2[r] = (float)(s + (double)k2->Tcw.at<float>(r, 3));
    }
    const float invz = 1.0f / C2[2];
    ex = k2->fx * C2[0] * invz + k2->cx;
    ey = k2->fy * C2[1] * invz + k2->cy;
}

struct Flat {
    std::vector<uint8_t> desc, skip;
    std::vector<int32_t> node, off, idx;
    explicit Flat(KeyFrame *k) : desc((size_t)k->N * 32), skip(k->N)
    {
        for (int i = 0; i < k->N; i++) {
            memcpy(&desc[(size_t)i * 32], k->mDescriptors.ptr(i), 32);
            skip[i] = k->mvpMapPoints[i] ? 1 : 0;
        }
        off.push_back(0);
        for (DBoW2::FeatureVector::const_iterator it = k->mFeatVec.begin(); it != k->mFeatVec.end(); ++it) {
            node.push_back((int32_t)it->first);
            for (size_t j = 0; j < it->second.size(); j++) idx.push_back((int32_t)it->second[j]);
            off.push_back((int32_t)idx.size());
        }
    }
};

static int expect(KeyFrame *k1, KeyFrame *k2, const cv::Mat &F12, bool onlyStereo, bool checkOri, Pairs &pairs)
{
    pairs.clear();
    if (k1->N == 0 || k2->N == 0) return 0;
    const Flat a(k1), b(k2);
    float F[9], ex, ey;
    for (int i = 0; i < 9; i++) F[i] = F12.at<float>(i / 3, i % 3);
    epipole(k1, k2, ex, ey);
    std::vector<int32_t> m12(k1->N);
    const int nm = tri::flat_search(
        reinterpret_cast<const tri::Kp *>(k1->mvKeysUn.data()), a.desc.data(), k1->N, a.skip.data(),
        (int)k1->mvuRight.size() == k1->N ? k1->mvuRight.data() : NULL, a.node.data(), a.off.data(), a.idx.data(), (int)a.node.size(),
        reinterpret_cast<const tri::Kp *>(k2->mvKeysUn.data()), b.desc.data(), b.skip.data(),
        (int)k2->mvuRight.size() == k2->N ? k2->mvuRight.data() : NULL, b.node.data(), b.off.data(), b.idx.data(), (int)b.node.size(), F,
        ex, ey, k2->mvScaleFactors.data(), k2->mvLevelSigma2.data(), onlyStereo, checkOri, m12.data());
    for (int i = 0; i < k1->N; i++)
        if (m12[i] >= 0) pairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
    return nm;
}

// one call through the class, compared neighbour by neighbour; returns the number of matches
static int run(TriangulationSearch &ts, KeyFrame *k1, const std::vector<KeyFrame *> &nb, const std::vector<cv::Mat> &F12, bool onlyStereo,
               bool checkOri, int atLeast)
{
    std::vector<Pairs> got;
    const int total = ts.SearchForTriangulation(k1, nb, F12, got, onlyStereo, checkOri);
    CHECK(got.size() == nb.size());
    int sum = 0;
    for (size_t k = 0; k < nb.size(); k++) {
        Pairs want;
        sum += expect(k1, nb[k], F12[k], onlyStereo, checkOri, want);
        CHECK(got[k] == want);
        for (size_t j = 1; j < got[k].size(); j++) CHECK(got[k][j - 1].first < got[k][j].first);   // ascending idx1
    }
    printf("  %d neighbours, only_stereo %d, check_ori %d: %d matches\n", (int)nb.size(), (int)onlyStereo, (int)checkOri, total);
    CHECK(total == sum);
    CHECK(total >= atLeast);
    return total;
}

int main()
{
    const int K = 6;
    tri::Scene S;
    tri::make_scene(S, K, 320, 11, [](int k) { return k == 3 ? 0 : k == 5 ? 2 : 1; });   // stereo views, one without mvuRight, one with -1s
    MockLog &L = mock_log();
    {
        TriangulationSearch ts;
        ts.SetResidentSetLimit(4);
        CHECK(L.limits.size() == 1 && L.limits[0] == 4);

        // 1. the first call: seven sets for a table of four -- the class asks for the limit it needs; every key frame is put once
        const int first = run(ts, &S.kf[0], S.nb, S.F12, false, true, 300);
        CHECK(L.limits.size() == 2 && L.limits[1] == K + 1);
        CHECK(L.puts.size() == (size_t)K + 1 && mock_resident() == K + 1 && L.searches == 1);
        for (int k = 1; k <= K; k++) CHECK(std::count(L.puts.begin(), L.puts.end(), (uint64_t)S.kf[k].mnId + 1) == 1);
        // the records: keys and epipoles in neighbour order, the flags concatenated in neighbour order, -1 for the view without mvuRight
        CHECK(L.nb.size() == (size_t)K && !L.ur1Null && !L.ur2Null);
        size_t at = 0;
        for (int k = 0; k < K; k++) {
            KeyFrame *p = S.nb[k];
            float ex, ey;
            epipole(&S.kf[0], p, ex, ey);
            CHECK(L.nb[k].key2 == (uint64_t)p->mnId + 1 && L.nb[k].ex == ex && L.nb[k].ey == ey);
            for (int i = 0; i < 9; i++) CHECK(L.nb[k].F12[i] == S.F12[k].at<float>(i / 3, i % 3));
            for (int i = 0; i < p->N; i++) {
                CHECK(L.skip2[at + i] == (p->mvpMapPoints[i] ? 1 : 0));
                CHECK(L.ur2[at + i] == (p->mvuRight.empty() ? -1.0f : p->mvuRight[i]));
            }
            at += (size_t)p->N;
        }
        CHECK(L.skip2.size() == at);

        // 2. the same call again: every set is a hit, nothing is put
        run(ts, &S.kf[0], S.nb, S.F12, false, true, first);
        CHECK(L.puts.size() == (size_t)K + 1 && L.searches == 2);
        run(ts, &S.kf[0], S.nb, S.F12, true, false, 90);   // only stereo pairs, no orientation check
        CHECK(L.puts.size() == (size_t)K + 1);

        // 3. map points change: the flags travel, the sets stay
        for (int i = 0; i < S.kf[0].N; i += 3) S.kf[0].mvpMapPoints[i] = S.kf[0].mvpMapPoints[i] ? NULL : &S.points[0];
        for (int i = 0; i < S.kf[2].N; i += 2) S.kf[2].mvpMapPoints[i] = S.kf[2].mvpMapPoints[i] ? NULL : &S.points[1];
        const int changed = run(ts, &S.kf[0], S.nb, S.F12, false, true, 220);
        CHECK(changed != first && L.puts.size() == (size_t)K + 1);

        // 4. an id handed out again (Tracking::Reset restarts KeyFrame::nNextId): other features under the id of neighbour 2
        KeyFrame reused(S.kf[5]);
        reused.mnId = S.kf[3].mnId;
        std::vector<KeyFrame *> nb = S.nb;
        nb[2] = &reused;
        run(ts, &S.kf[0], nb, S.F12, false, true, 180);
        CHECK(L.puts.size() == (size_t)K + 2 && L.puts.back() == (uint64_t)S.kf[3].mnId + 1);

        // 5. a key frame met before ComputeBoW: no FeatureVector, no matches; put again once it has one
        KeyFrame late(S.kf[1]);
        late.mnId = KeyFrame::NextId()++;
        const DBoW2::FeatureVector fv = late.mFeatVec;
        late.mFeatVec.clear();
        std::vector<KeyFrame *> one(1, &late);
        std::vector<cv::Mat> oneF(1, S.F12[0]);
        std::vector<Pairs> got;
        CHECK(ts.SearchForTriangulation(&S.kf[0], one, oneF, got, false, true) == 0 && got.size() == 1 && got[0].empty());
        const size_t puts = L.puts.size();
        late.mFeatVec = fv;
        run(ts, &S.kf[0], one, oneF, false, true, 20);
        CHECK(L.puts.size() == puts + 1);

        // 6. a key frame twice under two F12, key frame 1 as its own neighbour, a neighbour without features in between
        KeyFrame empty;
        empty.mvScaleFactors = S.kf[1].mvScaleFactors;
        empty.mvLevelSigma2 = S.kf[1].mvLevelSigma2;
        std::vector<KeyFrame *> mix;
        std::vector<cv::Mat> mixF;
        mix.push_back(&S.kf[1]); mixF.push_back(S.F12[0]);
        mix.push_back(&empty);   mixF.push_back(S.F12[1]);
        mix.push_back(&S.kf[1]); mixF.push_back(S.F12[2]);
        mix.push_back(&S.kf[0]); mixF.push_back(S.F12[0]);
        run(ts, &S.kf[0], mix, mixF, false, false, 250);
        CHECK(L.nb.size() == 3);                              // the empty key frame is not sent

        // 7. Tracking::Reset
        ts.DropResidentSets();
        CHECK(L.drops == 1 && mock_resident() == 0);
        const size_t before = L.puts.size();
        run(ts, &S.kf[0], S.nb, S.F12, false, true, 220);
        CHECK(L.puts.size() == before + K + 1);

        // 8. failures: reported, counted, nothing thrown, empty lists
        const unsigned long errs = OrbHipErrorCount();
        std::vector<cv::Mat> shortF(S.F12.begin(), S.F12.begin() + 2);
        CHECK(ts.SearchForTriangulation(&S.kf[0], S.nb, shortF, got, false, true) == 0 && got.size() == S.nb.size() && got[0].empty());
        S.kf[4].mvScaleFactors[3] = 2.f;                      // a neighbour with level tables of its own
        CHECK(ts.SearchForTriangulation(&S.kf[0], S.nb, S.F12, got, false, true) == 0 && got[1].empty());
        CHECK(OrbHipErrorCount() == errs + 2);
        // no neighbours, no features: nothing to do, no error
        CHECK(ts.SearchForTriangulation(&S.kf[0], std::vector<KeyFrame *>(), std::vector<cv::Mat>(), got, false, true) == 0 && got.empty());
        CHECK(OrbHipErrorCount() == errs + 2);
    }
    printf("test_trisearch_mock: OK (%d checks)\n", g_checks);
    return 0;
}
