// ORB_SLAM2::RansacScore (one device call per solver) against the loops it replaces, restated on the host (host_loops.h): every
// hypothesis's count, the records / the winner of the iterate() bookkeeping and their inlier flags.
//   test_ransac_dropin <scene.bin> <out.bin>
// out.bin, as the class returned it -- after this program found it equal to its own restatement --
//   PnP:  int32 0, N, M, nRecords, nBestOut, nKept; counts [M]; nKept indices; nKept counts; nKept x N flag bytes
//   Sim3: int32 1, N, M, nWinner, nInliers, nBestIt, nBestOut; counts [M]; N flag bytes
#include <algorithm>
#include <cstdio>
#include <vector>

#include "RansacScore.h"
#include "hiperror.h"
#include "host_loops.h"
#include "scene_io.h"

using namespace ORB_SLAM2;

namespace
{
cv::Mat column(const float *p, int n)
{
    cv::Mat m(n, 1, CV_32F);
    for (int k = 0; k < n; k++) m.at<float>(k, 0) = p[k];
    return m;
}
cv::Mat calibration(const float *K)
{
    cv::Mat m = cv::Mat::zeros(3, 3, CV_32F);
    m.at<float>(0, 0) = K[0], m.at<float>(1, 1) = K[1], m.at<float>(0, 2) = K[2], m.at<float>(1, 2) = K[3], m.at<float>(2, 2) = 1.f;
    return m;
}
cv::Mat transform(const float *T34)
{
    cv::Mat m = cv::Mat::zeros(4, 4, CV_32F);
    for (int k = 0; k < 12; k++) m.at<float>(k / 4, k % 4) = T34[k];
    m.at<float>(3, 3) = 1.f;
    return m;
}

int run_pnp(const Scene &s, const char *dst)
{
    const int N = s.N, M = s.M;
    std::vector<cv::Point3f> P3Dw(N);
    std::vector<cv::Point2f> P2D(N);
    for (int i = 0; i < N; i++) {
        P3Dw[i] = cv::Point3f(s.P3Dw[3 * i], s.P3Dw[3 * i + 1], s.P3Dw[3 * i + 2]);
        P2D[i] = cv::Point2f(s.P2D[2 * i], s.P2D[2 * i + 1]);
    }
    std::vector<std::array<double, 9> > vR(M);
    std::vector<std::array<double, 3> > vt(M);
    for (int h = 0; h < M; h++) {
        for (int k = 0; k < 9; k++) vR[h][k] = s.Rt[12 * h + k];
        for (int k = 0; k < 3; k++) vt[h][k] = s.Rt[12 * h + 9 + k];
    }
    RansacScore scorer;
    RansacScore::PnPResult R;
    if (!scorer.ScorePnP(P3Dw, P2D, s.maxErr, s.cam[0], s.cam[1], s.cam[2], s.cam[3], vR, vt, s.minInliers, s.bestIn, R) || OrbHipErrorCount())
    { fprintf(stderr, "RansacScore::ScorePnP failed: %s\n", OrbHipLastError()); return 1; }

    // the restatement: iterate()'s loop, keeping mvbBestInliers at every record
    std::vector<int> counts(M), idx(M), cnt(M);
    std::vector<unsigned char> cur(N), bestFlags(N);
    int best = s.bestIn;
    const int nrec = pnp_iterate(s.Rt.data(), M, s.P3Dw.data(), s.P2D.data(), s.maxErr.data(), N, s.cam[0], s.cam[1], s.cam[2], s.cam[3],
                                 s.minInliers, &best, counts.data(), idx.data(), cnt.data(), cur.data(), bestFlags.data());
    const int kept = (int)R.vnRecordIt.size();
    if (R.nRecords != nrec || R.nBestOut != best || kept != std::min(nrec, (int)RansacScore::kMaxRecords) || (int)R.vnInliers.size() != M ||
        (int)R.vnRecordInliers.size() != kept || (int)R.vvbRecordInliers.size() != kept)
    { fprintf(stderr, "PnP: %d records, best %d; the class returned %d, %d (%d kept)\n", nrec, best, R.nRecords, R.nBestOut, kept); return 1; }
    for (int h = 0; h < M; h++)
        if (R.vnInliers[h] != counts[h]) { fprintf(stderr, "PnP hypothesis %d: %d inliers, the class returned %d\n", h, counts[h], R.vnInliers[h]); return 1; }
    std::vector<unsigned char> flagBytes;
    for (int r = 0; r < kept; r++) {
        if (R.vnRecordIt[r] != idx[r] || R.vnRecordInliers[r] != cnt[r]) { fprintf(stderr, "PnP record %d: (%d, %d), the class returned (%d, %d)\n", r, idx[r], cnt[r], R.vnRecordIt[r], R.vnRecordInliers[r]); return 1; }
        pnp_check_inliers(s.Rt.data() + 12 * idx[r], s.P3Dw.data(), s.P2D.data(), s.maxErr.data(), N, s.cam[0], s.cam[1], s.cam[2], s.cam[3], cur.data());
        if ((int)R.vvbRecordInliers[r].size() != N) { fprintf(stderr, "PnP record %d: %zu flags\n", r, R.vvbRecordInliers[r].size()); return 1; }
        for (int i = 0; i < N; i++) {
            if (R.vvbRecordInliers[r][i] != (cur[i] != 0)) { fprintf(stderr, "PnP record %d: other inliers (point %d)\n", r, i); return 1; }
            flagBytes.push_back(cur[i]);
        }
    }
    const int head[6] = {0, N, M, R.nRecords, R.nBestOut, kept};
    FILE *o = fopen(dst, "wb");
    const bool ok = o && put(o, head, 24) && put(o, R.vnInliers.data(), (size_t)M * 4) && put(o, R.vnRecordIt.data(), (size_t)kept * 4) &&
                    put(o, R.vnRecordInliers.data(), (size_t)kept * 4) && put(o, flagBytes.data(), flagBytes.size());
    if (!ok || fclose(o)) { perror(dst); return 2; }
    printf("ok pnp %d %d %d\n", N, M, R.nRecords);
    return 0;
}

int run_sim3(const Scene &s, const char *dst)
{
    const int N = s.N, M = s.M;
    std::vector<cv::Mat> X1, X2, p1, p2, vT12, vT21;
    for (int i = 0; i < N; i++) {
        X1.push_back(column(s.X1.data() + 3 * i, 3)), X2.push_back(column(s.X2.data() + 3 * i, 3));
        p1.push_back(column(s.p1.data() + 2 * i, 2)), p2.push_back(column(s.p2.data() + 2 * i, 2));
    }
    for (int h = 0; h < M; h++) vT12.push_back(transform(s.T.data() + 24 * h)), vT21.push_back(transform(s.T.data() + 24 * h + 12));
    RansacScore scorer;
    RansacScore::Sim3Result R;
    if (!scorer.ScoreSim3(X1, X2, p1, p2, s.maxErr1, s.maxErr2, calibration(s.K1), calibration(s.K2), vT12, vT21, s.minInliers, s.bestIn, R) ||
        OrbHipErrorCount())
    { fprintf(stderr, "RansacScore::ScoreSim3 failed: %s\n", OrbHipLastError()); return 1; }

    std::vector<int> counts(M, -1);
    std::vector<unsigned char> cur(N), bestFlags(N);
    int best = s.bestIn, bestIt;
    const int w = sim3_iterate(s.T.data(), M, s.X1.data(), s.X2.data(), s.p1.data(), s.p2.data(), s.maxErr1.data(), s.maxErr2.data(), N, s.K1,
                               s.K2, s.minInliers, &best, &bestIt, counts.data(), cur.data(), bestFlags.data());
    if (R.nWinner != w || R.nBestIt != bestIt || R.nBestOut != best || R.nInliers != (w >= 0 ? counts[w] : 0) || (int)R.vbInliers.size() != N ||
        (int)R.vnInliers.size() != M)
    { fprintf(stderr, "Sim3: winner %d, best %d at %d; the class returned %d, %d at %d\n", w, best, bestIt, R.nWinner, R.nBestOut, R.nBestIt); return 1; }
    for (int h = 0; h < M && counts[h] >= 0; h++)                          // (the loop stopped at the winner)
        if (R.vnInliers[h] != counts[h]) { fprintf(stderr, "Sim3 hypothesis %d: %d inliers, the class returned %d\n", h, counts[h], R.vnInliers[h]); return 1; }
    std::vector<unsigned char> flagBytes(N);
    for (int i = 0; i < N; i++) {
        flagBytes[i] = R.vbInliers[i];
        if (R.vbInliers[i] != (w >= 0 && bestFlags[i] != 0)) { fprintf(stderr, "Sim3: other inliers (point %d)\n", i); return 1; }
    }
    const int head[7] = {1, N, M, R.nWinner, R.nInliers, R.nBestIt, R.nBestOut};
    FILE *o = fopen(dst, "wb");
    const bool ok = o && put(o, head, 28) && put(o, R.vnInliers.data(), (size_t)M * 4) && put(o, flagBytes.data(), N);
    if (!ok || fclose(o)) { perror(dst); return 2; }
    printf("ok sim3 %d %d %d\n", N, M, R.nWinner);
    return 0;
}
}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]); return 2; }
    Scene s;
    if (!read_scene(argv[1], s)) return 2;
    return s.kind == 0 ? run_pnp(s, argv[2]) : run_sim3(s, argv[2]);
}
