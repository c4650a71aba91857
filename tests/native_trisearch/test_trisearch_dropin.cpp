// test_trisearch_dropin.cpp -- on the device: ORB_SLAM2::TriangulationSearch over K key frames must fill, neighbour by neighbour,
// what K calls of ORBmatcher::SearchForTriangulation fill (LocalMapping::CreateNewMapPoints, ref: src/LocalMapping.cc:2258-2298).
// Monocular and stereo key frames; a second call after map points changed (the flags travel, the sets do not); a call after an
// id was handed out again (the fingerprint makes the set be put again).
#include <cstdio>
#include <cstdlib>

#include "ORBmatcher.h"
#include "TriangulationSearch.h"
#include "hiperror.h"
#include "tri_scene.h"

using namespace ORB_SLAM2;
typedef std::vector<std::pair<size_t, size_t> > Pairs;

static int g_checks = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checks++;                                                                      \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static int run(TriangulationSearch &ts, KeyFrame *k1, const std::vector<KeyFrame *> &nb, const std::vector<cv::Mat> &F12, bool onlyStereo,
               bool checkOri, int atLeast)
{
    std::vector<Pairs> got;
    const int total = ts.SearchForTriangulation(k1, nb, F12, got, onlyStereo, checkOri);
    CHECK(got.size() == nb.size());
    ORBmatcher matcher(0.6, checkOri);
    int sum = 0;
    for (size_t k = 0; k < nb.size(); k++) {
        Pairs want;
        sum += matcher.SearchForTriangulation(k1, nb[k], F12[k], want, onlyStereo);
        CHECK(got[k] == want);
    }
    printf("  %d neighbours, only_stereo %d, check_ori %d: %d matches\n", (int)nb.size(), (int)onlyStereo, (int)checkOri, total);
    CHECK(total == sum);
    CHECK(total >= atLeast);
    CHECK(OrbHipErrorCount() == 0);
    return total;
}

// (the lower bounds: about two thirds of what the host model of tests/native_trisearch/mock_trisearch.cc counts on these scenes --
// 1256 / 1177 / 1029 / 1020 / 567 monocular, 1181 / 1099 / 381 / 892 / 895 / 487 stereo, in the order of the calls)
int main()
{
    const int K = 10;
    for (int stereo = 0; stereo < 2; stereo++) {
        tri::Scene S;
        // monocular key frames as the reference fills them (mvuRight of -1) / stereo ones, one of them without mvuRight
        tri::make_scene(S, K, 600, 21 + stereo, [stereo](int k) { return stereo ? (k == 4 ? 0 : 1) : 2; });
        TriangulationSearch ts;
        const int first = run(ts, &S.kf[0], S.nb, S.F12, false, false, 800);   // ORBmatcher(0.6, false): what CreateNewMapPoints constructs
        run(ts, &S.kf[0], S.nb, S.F12, false, true, 600);
        if (stereo) run(ts, &S.kf[0], S.nb, S.F12, true, false, 200);
        // map points change on both sides
        for (int i = 0; i < S.kf[0].N; i += 3) S.kf[0].mvpMapPoints[i] = S.kf[0].mvpMapPoints[i] ? NULL : &S.points[0];
        for (int i = 0; i < S.kf[2].N; i += 2) S.kf[2].mvpMapPoints[i] = S.kf[2].mvpMapPoints[i] ? NULL : &S.points[1];
        CHECK(run(ts, &S.kf[0], S.nb, S.F12, false, false, 600) != first);
        // the id of neighbour 2 handed out again, with the features of neighbour 6
        KeyFrame reused(S.kf[7]);
        reused.mnId = S.kf[3].mnId;
        std::vector<KeyFrame *> nb = S.nb;
        nb[2] = &reused;
        run(ts, &S.kf[0], nb, S.F12, false, false, 600);
        // a key frame twice under two F12, key frame 1 as its own neighbour
        std::vector<KeyFrame *> mix;
        std::vector<cv::Mat> mixF;
        mix.push_back(&S.kf[1]); mixF.push_back(S.F12[0]);
        mix.push_back(&S.kf[1]); mixF.push_back(S.F12[2]);
        mix.push_back(&S.kf[0]); mixF.push_back(S.F12[0]);
        run(ts, &S.kf[0], mix, mixF, false, true, 200);
    }
    printf("test_trisearch_dropin: OK (%d checks)\n", g_checks);
    return 0;
}
