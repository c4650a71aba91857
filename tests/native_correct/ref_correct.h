// ref_correct.h -- the two loops of the reference written out on slamlite.h objects, for the twin map of test_correct.cpp:
// LoopClosing::CorrectLoop's pass over CorrectedSim3 (ref: src/LoopClosing.cc:523-568, without UpdateConnections) and the point loop of
// LoopClosing::RunGlobalBundleAdjustment (ref: :762-797).  g2o::Sim3::map is s*(r*xyz)+t with Eigen 3's Quaternion::_transformVector
// (docs/parity.md, "CorrectLoop"); the programs are built with -ffp-contract=off, so every operation below is rounded on its own.
#ifndef ORBHIP_TESTS_REF_CORRECT_H
#define ORBHIP_TESTS_REF_CORRECT_H
#include <vector>

#include "LocalMap.h"

namespace refcorrect
{
using namespace ORB_SLAM2;
typedef LocalMapSearch::Sim3d Sim3d;

inline void cross(const double a[3], const double b[3], double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// Sim3::map
inline void map(const Sim3d &S, const double xyz[3], double out[3])
{
    double uv[3], c[3];
    cross(S.q, xyz, uv);                       // Vector3 uv = this->vec().cross(v);
    for (int i = 0; i < 3; i++) uv[i] += uv[i];   // uv += uv;
    cross(S.q, uv, c);
    for (int i = 0; i < 3; i++) {
        const double r = (xyz[i] + S.q[3] * uv[i]) + c[i];   // return v + this->w() * uv + this->vec().cross(uv);
        out[i] = S.s * r + S.t[i];
    }
}

inline cv::Mat mat3(const float *p)
{
    cv::Mat m(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) m.at<float>(c, 0) = p[c];
    return m;
}

inline int correct_loop(const std::vector<LocalMapSearch::LoopCorrection> &CorrectedSim3, unsigned long nCurrentKFid)
{
    int moved = 0;
    for (size_t k = 0; k < CorrectedSim3.size(); k++) {
        KeyFrame *pKFi = CorrectedSim3[k].pKF;
        std::vector<MapPoint *> vpMPsi = pKFi->GetMapPointMatches();
        for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
            MapPoint *pMPi = vpMPsi[iMP];
            if (!pMPi) continue;
            if (pMPi->isBad()) continue;
            if (pMPi->mnCorrectedByKF == nCurrentKFid) continue;
            cv::Mat P3Dw = pMPi->GetWorldPos();
            const double eigP3Dw[3] = {P3Dw.at<float>(0, 0), P3Dw.at<float>(1, 0), P3Dw.at<float>(2, 0)};
            double mid[3], eigCorrectedP3Dw[3];
            map(CorrectedSim3[k].Siw, eigP3Dw, mid);
            map(CorrectedSim3[k].correctedSwi, mid, eigCorrectedP3Dw);
            const float f[3] = {(float)eigCorrectedP3Dw[0], (float)eigCorrectedP3Dw[1], (float)eigCorrectedP3Dw[2]};
            pMPi->SetWorldPos(mat3(f));
            pMPi->mnCorrectedByKF = nCurrentKFid;
            pMPi->mnCorrectedReference = pKFi->mnId;
            pMPi->UpdateNormalAndDepth();
            moved++;
        }
        pKFi->SetPose(CorrectedSim3[k].correctedTiw);
    }
    return moved;
}

// cv::Mat R*x + t on CV_32F: one gemm, summed in double from 0.0, t added, one rounding
inline void gemm3(const cv::Mat &T, const float x[3], float out[3])
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)T.at<float>(r, k) * (double)x[k];
        out[r] = (float)(s + (double)T.at<float>(r, 3));
    }
}

inline int global_ba(const std::vector<MapPoint *> &vpMPs, unsigned long nLoopKF)
{
    int moved = 0;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        if (pMP->mnBAGlobalForKF == nLoopKF) {
            pMP->SetWorldPos(pMP->mPosGBA);
        } else {
            KeyFrame *pRefKF = pMP->GetReferenceKeyFrame();
            if (pRefKF->mnBAGlobalForKF != nLoopKF) continue;
            const cv::Mat X = pMP->GetWorldPos();
            const float xw[3] = {X.at<float>(0, 0), X.at<float>(1, 0), X.at<float>(2, 0)};
            float Xc[3], out[3];
            gemm3(pRefKF->mTcwBefGBA, xw, Xc);
            gemm3(pRefKF->GetPoseInverse(), Xc, out);
            pMP->SetWorldPos(mat3(out));
        }
        moved++;
    }
    return moved;
}
}  // namespace refcorrect

#endif
