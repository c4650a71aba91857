// InitializerScore.cc -- host side of ORB_SLAM2::InitializerScore (include/orbhip/InitializerScore.h): packs the hypotheses of
// all RANSAC iterations, makes the one orbhip_init_score call and compacts the inlier bytes, which the library returns per
// frame-1 feature, into mvMatches12 order (ref: src/Initializer.cc:54-63).
#include "InitializerScore.h"

#include <cstdint>

#include "hiperror.h"
#include "orbhip.h"

namespace ORB_SLAM2
{

namespace
{
int g_initscore_device = 0;

// 3x3 CV_32F matrices -> [n][9] row-major; false: one of them is something else
bool pack(const std::vector<cv::Mat> &v, std::vector<float> &out)
{
    out.resize(9 * v.size());
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].rows != 3 || v[i].cols != 3 || v[i].type() != CV_32F) return false;
        for (int k = 0; k < 9; k++) out[9 * i + k] = v[i].at<float>(k / 3, k % 3);
    }
    return true;
}
}  // namespace

void InitializerScore::SetDevice(int device) { g_initscore_device = device; }

InitializerScore::InitializerScore() : mpCtx(NULL)
{
    mpCtx = orbhip_create(g_initscore_device, 50, 1.2f, 1, 20, 7, 128, 128, 1);   // the smallest context: only its stream is used
    if (!mpCtx) hipdetail::Fail("InitializerScore (device context)", orbhip_last_error(NULL));
}

InitializerScore::~InitializerScore()
{
    if (mpCtx) orbhip_destroy(mpCtx);
}

bool InitializerScore::Score(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2,
                             const std::vector<int> &vMatches12, const std::vector<cv::Mat> &vH21, const std::vector<cv::Mat> &vH12,
                             const std::vector<cv::Mat> &vF21, float sigma, Result &out)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return hipdetail::Fail("InitializerScore::Score", "no device context");
    if (vMatches12.size() != vKeys1.size() || vH21.size() != vH12.size())
        return hipdetail::Fail("InitializerScore::Score", "vMatches12 must have one entry per key of frame 1, vH12 one per vH21");
    std::vector<float> h21, h12, f21;
    if (!pack(vH21, h21) || !pack(vH12, h12) || !pack(vF21, f21))
        return hipdetail::Fail("InitializerScore::Score", "a hypothesis is not a 3x3 CV_32F matrix");
    const int n1 = (int)vKeys1.size(), nH = (int)vH21.size(), nF = (int)vF21.size();
    std::vector<int32_t> match(vMatches12.begin(), vMatches12.end());
    std::vector<float> scores(nH + nF);
    std::vector<uint8_t> inl(2 * (size_t)n1);
    orbhip_init_best best[2];
    const int rc = orbhip_init_score(mpCtx, reinterpret_cast<const orbhip_keypoint *>(vKeys1.data()), n1,
                                     reinterpret_cast<const orbhip_keypoint *>(vKeys2.data()), (int)vKeys2.size(), match.data(),
                                     h21.data(), h12.data(), nH, f21.data(), nF, sigma, scores.data(), best, inl.data());
    if (rc != ORBHIP_OK) return hipdetail::Fail("InitializerScore::Score", orbhip_last_error(mpCtx));
    out.SH = best[0].score, out.itH = best[0].it;
    out.SF = best[1].score, out.itF = best[1].it;
    out.vScoresH.assign(scores.begin(), scores.begin() + nH);
    out.vScoresF.assign(scores.begin() + nH, scores.end());
    out.vbMatchesInliersH.clear();
    out.vbMatchesInliersF.clear();
    for (int i = 0; i < n1; i++)
        if (vMatches12[i] >= 0) {                                // mvMatches12: the matched features of frame 1 in index order
            out.vbMatchesInliersH.push_back(inl[i] != 0);
            out.vbMatchesInliersF.push_back(inl[(size_t)n1 + i] != 0);
        }
    return true;
}

}  // namespace ORB_SLAM2
