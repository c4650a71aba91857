// RansacScore.cc -- host side of ORB_SLAM2::RansacScore (include/orbhip/RansacScore.h): packs the correspondences and the
// hypotheses of a round, makes the one orbhip_pnp_score / orbhip_sim3_score call and unpacks the records / the winner.
#include "RansacScore.h"

#include <algorithm>
#include <cstdint>

#include "hiperror.h"
#include "orbhip.h"

namespace ORB_SLAM2
{

namespace
{
int g_ransac_device = 0;

// n x 1 CV_32F matrices -> [count][n]; false: one of them is something else
bool pack_cols(const std::vector<cv::Mat> &v, int n, std::vector<float> &out)
{
    out.resize((size_t)n * v.size());
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].rows != n || v[i].cols != 1 || v[i].type() != CV_32F) return false;
        for (int k = 0; k < n; k++) out[n * i + k] = v[i].at<float>(k, 0);
    }
    return true;
}

// {fx, fy, cx, cy} of a 3x3 CV_32F calibration matrix
bool pack_K(const cv::Mat &K, float out[4])
{
    if (K.rows != 3 || K.cols != 3 || K.type() != CV_32F) return false;
    out[0] = K.at<float>(0, 0), out[1] = K.at<float>(1, 1), out[2] = K.at<float>(0, 2), out[3] = K.at<float>(1, 2);
    return true;
}
}  // namespace

void RansacScore::SetDevice(int device) { g_ransac_device = device; }

RansacScore::RansacScore() : mpCtx(NULL)
{
    mpCtx = orbhip_create(g_ransac_device, 50, 1.2f, 1, 20, 7, 128, 128, 1);   // the smallest context: only its stream is used
    if (!mpCtx) hipdetail::Fail("RansacScore (device context)", orbhip_last_error(NULL));
}

RansacScore::~RansacScore()
{
    if (mpCtx) orbhip_destroy(mpCtx);
}

bool RansacScore::ScorePnP(const std::vector<cv::Point3f> &vP3Dw, const std::vector<cv::Point2f> &vP2D, const std::vector<float> &vMaxError,
                           double fu, double fv, double uc, double vc, const std::vector<std::array<double, 9> > &vR,
                           const std::vector<std::array<double, 3> > &vt, int minInliers, int bestIn, PnPResult &out)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return hipdetail::Fail("RansacScore::ScorePnP", "no device context");
    if (vP2D.size() != vP3Dw.size() || vMaxError.size() != vP3Dw.size() || vt.size() != vR.size())
        return hipdetail::Fail("RansacScore::ScorePnP", "vP2D and vMaxError must have one entry per point of vP3Dw, vt one per vR");
    const int N = (int)vP3Dw.size(), M = (int)vR.size();
    std::vector<float> X(3 * (size_t)N), uv(2 * (size_t)N);
    for (int i = 0; i < N; i++) {
        X[3 * i] = vP3Dw[i].x, X[3 * i + 1] = vP3Dw[i].y, X[3 * i + 2] = vP3Dw[i].z;
        uv[2 * i] = vP2D[i].x, uv[2 * i + 1] = vP2D[i].y;
    }
    std::vector<double> Rt(12 * (size_t)M);
    for (int h = 0; h < M; h++) {
        std::copy(vR[h].begin(), vR[h].end(), Rt.begin() + 12 * h);
        std::copy(vt[h].begin(), vt[h].end(), Rt.begin() + 12 * h + 9);
    }
    const int R = std::max(1, std::min(M, (int)kMaxRecords));
    std::vector<int32_t> counts(M), idx(R), cnt(R);
    std::vector<uint8_t> flags((size_t)R * N);
    orbhip_pnp_result res;
    const int rc = orbhip_pnp_score(mpCtx, X.data(), uv.data(), vMaxError.data(), N, fu, fv, uc, vc, Rt.data(), M, minInliers, bestIn, R,
                                    counts.data(), &res, idx.data(), cnt.data(), flags.data());
    if (rc != ORBHIP_OK) return hipdetail::Fail("RansacScore::ScorePnP", orbhip_last_error(mpCtx));
    const int n = std::min(res.n_records, R);
    out.nRecords = res.n_records, out.nBestOut = res.best_out;
    out.vnRecordIt.assign(idx.begin(), idx.begin() + n);
    out.vnRecordInliers.assign(cnt.begin(), cnt.begin() + n);
    out.vvbRecordInliers.assign(n, std::vector<bool>(N));
    for (int r = 0; r < n; r++)
        for (int i = 0; i < N; i++) out.vvbRecordInliers[r][i] = flags[(size_t)r * N + i] != 0;
    out.vnInliers.assign(counts.begin(), counts.end());
    return true;
}

bool RansacScore::ScoreSim3(const std::vector<cv::Mat> &vX3Dc1, const std::vector<cv::Mat> &vX3Dc2, const std::vector<cv::Mat> &vP1im1,
                            const std::vector<cv::Mat> &vP2im2, const std::vector<float> &vMaxError1, const std::vector<float> &vMaxError2,
                            const cv::Mat &K1, const cv::Mat &K2, const std::vector<cv::Mat> &vT12, const std::vector<cv::Mat> &vT21,
                            int minInliers, int bestIn, Sim3Result &out)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return hipdetail::Fail("RansacScore::ScoreSim3", "no device context");
    const size_t n = vX3Dc1.size();
    if (vX3Dc2.size() != n || vP1im1.size() != n || vP2im2.size() != n || vMaxError1.size() != n || vMaxError2.size() != n ||
        vT21.size() != vT12.size())
        return hipdetail::Fail("RansacScore::ScoreSim3", "the six point lists must have the same length, vT21 one entry per vT12");
    std::vector<float> X1, X2, p1, p2;
    float k1[4], k2[4];
    if (!pack_cols(vX3Dc1, 3, X1) || !pack_cols(vX3Dc2, 3, X2) || !pack_cols(vP1im1, 2, p1) || !pack_cols(vP2im2, 2, p2) ||
        !pack_K(K1, k1) || !pack_K(K2, k2))
        return hipdetail::Fail("RansacScore::ScoreSim3", "a point is not a 3x1 / 2x1 CV_32F matrix, or K not 3x3 CV_32F");
    const int N = (int)n, M = (int)vT12.size();
    std::vector<float> T(24 * (size_t)M);
    for (int h = 0; h < M; h++)
        for (int side = 0; side < 2; side++) {
            const cv::Mat &m = side ? vT21[h] : vT12[h];
            if (m.rows != 4 || m.cols != 4 || m.type() != CV_32F)
                return hipdetail::Fail("RansacScore::ScoreSim3", "a hypothesis is not a 4x4 CV_32F matrix");
            for (int k = 0; k < 12; k++) T[24 * h + 12 * side + k] = m.at<float>(k / 4, k % 4);
        }
    std::vector<int32_t> counts(M);
    std::vector<uint8_t> flags(N);
    orbhip_sim3_result res;
    const int rc = orbhip_sim3_score(mpCtx, X1.data(), X2.data(), p1.data(), p2.data(), vMaxError1.data(), vMaxError2.data(), N, k1, k2,
                                     T.data(), M, minInliers, bestIn, counts.data(), &res, flags.data());
    if (rc != ORBHIP_OK) return hipdetail::Fail("RansacScore::ScoreSim3", orbhip_last_error(mpCtx));
    out.nWinner = res.winner, out.nInliers = res.ninliers, out.nBestIt = res.best_it, out.nBestOut = res.best_out;
    out.vbInliers.assign(N, false);
    for (int i = 0; i < N; i++) out.vbInliers[i] = flags[i] != 0;
    out.vnInliers.assign(counts.begin(), counts.end());
    return true;
}

}  // namespace ORB_SLAM2
