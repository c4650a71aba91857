// RansacScore.h -- ORB_SLAM2::RansacScore: the CheckInliers calls of PnPsolver::iterate (ref: src/PnPsolver.cc:207-225 with
// CheckInliers :308-339) and Sim3Solver::iterate (src/Sim3Solver.cc:181-200 with CheckInliers + Project :340-403) for all the
// hypotheses the caller has, as one device call each (orbhip_pnp_score / orbhip_sim3_score; include/orbhip.h).
// No counterpart class in the reference: the solver draws its sets and runs compute_pose / ComputeSim3 for the iterations of a round
// first and hands the poses over.  Never throws; a failed device call is reported through
// hipdetail::Fail and the Score function returns false with nothing written (include/orbhip/hiperror.h).
//
// Arithmetic, every operation rounded on its own in the source's order.  PnP: R, t, fu, fv, uc, vc double, the point, the pixel and
// vMaxError float; Xc, Yc = (float) of the double row sums, invZc = (float)(1.0 / Zc) with a double division, ue = uc + ((fu * Xc) *
// invZc) in double, distX = (float)(u - ue), error2 = distX*distX + distY*distY in float, inlier iff error2 < vMaxError[i].  Sim3: all
// float; Project is one gemm (double accumulator from 0.0, + t, rounded once), invz = 1.0f / z, u = (fx * (x * invz)) + cx; the squared
// distances have Mat::dot's double accumulator; inlier iff err1 < vMaxError1[i] && err2 < vMaxError2[i].
#ifndef ORBHIP_RANSACSCORE_H
#define ORBHIP_RANSACSCORE_H

#include <array>
#include <mutex>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include <opencv2/opencv.hpp>
#else
#include "cvlite.h"
#ifndef ORBHIP_CVLITE_POINT3F
#define ORBHIP_CVLITE_POINT3F
namespace cv
{
template <typename T> struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T _x, T _y, T _z) : x(_x), y(_y), z(_z) {}
};
typedef Point3_<float> Point3f;
}  // namespace cv
#endif
#endif

struct orbhip_ctx;

namespace ORB_SLAM2
{

class RansacScore
{
public:
    RansacScore();                            // a device context of its own (a context is not re-entrant)
    ~RansacScore();
    RansacScore(const RansacScore &) = delete;
    RansacScore &operator=(const RansacScore &) = delete;

    enum { kMaxRecords = 64 };                // records returned with their flags per call; nRecords counts them all

    struct PnPResult
    {
        int nRecords;                         // hypotheses with count >= minInliers && count > the best before them
        int nBestOut;                         // mnBestInliers after the call: bestIn of the next chunk
        std::vector<int> vnRecordIt, vnRecordInliers;            // the first min(nRecords, kMaxRecords): index into vR, mnInliersi
        std::vector<std::vector<bool> > vvbRecordInliers;        // and mvbInliersi, one entry per correspondence
        std::vector<int> vnInliers;           // mnInliersi of every hypothesis
    };
    struct Sim3Result
    {
        int nWinner;                          // the first hypothesis with count >= best and count > minInliers; -1: none
        int nInliers;                         // its count (0 without a winner)
        int nBestIt, nBestOut;                // the last hypothesis that reached the best (-1: none of this call), mnBestInliers
        std::vector<bool> vbInliers;          // the winner's mvbInliersi (all false without one)
        std::vector<int> vnInliers;           // mnInliersi of every hypothesis; those behind the winner were not looked at by the rule
    };

    // vP3Dw / vP2D / vMaxError: mvP3Dw, mvP2D, mvMaxError; fu .. vc: the solver's doubles; vR[h] / vt[h]: mRi (row-major) and mti of
    // hypothesis h after compute_pose; minInliers: mRansacMinInliers; bestIn: mnBestInliers before the first of these hypotheses.
    bool ScorePnP(const std::vector<cv::Point3f> &vP3Dw, const std::vector<cv::Point2f> &vP2D, const std::vector<float> &vMaxError,
                  double fu, double fv, double uc, double vc, const std::vector<std::array<double, 9> > &vR,
                  const std::vector<std::array<double, 3> > &vt, int minInliers, int bestIn, PnPResult &out);

    // vX3Dc1 / vX3Dc2: 3x1 CV_32F; vP1im1 / vP2im2: 2x1 CV_32F; vMaxError1 / vMaxError2: what `err < mvnMaxError1[i]` compares with,
    // as float; K1 / K2: 3x3 CV_32F; vT12[h] / vT21[h]: mT12i / mT21i (4x4 CV_32F) of hypothesis h after ComputeSim3.
    bool ScoreSim3(const std::vector<cv::Mat> &vX3Dc1, const std::vector<cv::Mat> &vX3Dc2, const std::vector<cv::Mat> &vP1im1,
                   const std::vector<cv::Mat> &vP2im2, const std::vector<float> &vMaxError1, const std::vector<float> &vMaxError2,
                   const cv::Mat &K1, const cv::Mat &K2, const std::vector<cv::Mat> &vT12, const std::vector<cv::Mat> &vT21,
                   int minInliers, int bestIn, Sim3Result &out);

    // device of the objects constructed from now on (default 0)
    static void SetDevice(int device);

protected:
    orbhip_ctx *mpCtx;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
