// InitializerScore.h -- ORB_SLAM2::InitializerScore: the scoring half of Initializer::FindHomography / FindFundamental (ref:
// src/Initializer.cc:148-171, :199-222 with CheckHomography / CheckFundamental :305-468) as one device call
// (orbhip_init_score; include/orbhip.h).  No counterpart class in the reference: Initializer computes the
// H21i / H12i / F21i of all iterations first and hands them over.  Never throws; a failed device call
// is reported through hipdetail::Fail and Score returns false with nothing written (include/orbhip/hiperror.h).
#ifndef ORBHIP_INITIALIZERSCORE_H
#define ORBHIP_INITIALIZERSCORE_H

#include <mutex>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include <opencv2/opencv.hpp>
#else
#include "cvlite.h"
#endif

struct orbhip_ctx;

namespace ORB_SLAM2
{

class InitializerScore
{
public:
    InitializerScore();                       // a device context of its own (a context is not re-entrant)
    ~InitializerScore();
    InitializerScore(const InitializerScore &) = delete;
    InitializerScore &operator=(const InitializerScore &) = delete;

    struct Result
    {
        float SH, SF;                         // the winners' scores (0 when there is none)
        int itH, itF;                         // their iterations, -1: no hypothesis scored above 0
        std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;   // in mvMatches12 order: one entry per vMatches12[i] >= 0
        std::vector<float> vScoresH, vScoresF;                    // every iteration's score
    };

    // vKeys1 / vKeys2: mvKeys1 / mvKeys2 (undistorted); vMatches12: what SearchForInitialization returned; vH21 / vH12 / vF21:
    // 3x3 CV_32F, the arguments of the iterations' CheckHomography / CheckFundamental calls, in iteration order (either list may
    // be empty; vH12.size() == vH21.size()).
    bool Score(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2, const std::vector<int> &vMatches12,
               const std::vector<cv::Mat> &vH21, const std::vector<cv::Mat> &vH12, const std::vector<cv::Mat> &vF21, float sigma,
               Result &out);

    // device of the objects constructed from now on (default 0)
    static void SetDevice(int device);

protected:
    orbhip_ctx *mpCtx;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
