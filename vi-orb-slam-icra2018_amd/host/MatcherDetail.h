// MatcherDetail.h -- what the host sides of ORBmatcher (ORBmatcher.cc) and TriangulationSearch (triangulation/TriangulationSearch.cc)
// share: a key frame's data flattened for the C ABI, the identity rule of a resident set, the one-gemm affine map and the
// epipole of SearchForTriangulation.  Not installed: the public headers are under include/orbhip.
#ifndef ORBHIP_HOST_MATCHERDETAIL_H
#define ORBHIP_HOST_MATCHERDETAIL_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ORBmatcher.h"
#include "orbhip.h"

namespace ORB_SLAM2
{
namespace hipdetail
{

struct Csr {
    std::vector<int32_t> node, off, idx;
};
inline Csr flatten(const DBoW2::FeatureVector &fv)
{
    Csr c;
    c.off.push_back(0);
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        c.node.push_back((int32_t)it->first);
        for (size_t k = 0; k < it->second.size(); k++) c.idx.push_back((int32_t)it->second[k]);
        c.off.push_back((int32_t)c.idx.size());
    }
    return c;
}
inline std::vector<uint8_t> contiguous(const cv::Mat &d)
{
    std::vector<uint8_t> v((size_t)d.rows * 32);
    for (int i = 0; i < d.rows; i++) memcpy(&v[(size_t)i * 32], d.ptr(i), 32);
    return v;
}

// Is `key` of context c the resident set of t (a Frame or a KeyFrame)?  An id is not an identity: Tracking::Reset restarts
// KeyFrame::nNextId and Frame::nNextId (ref: src/Tracking.cc:2758-2759), and a key frame can be met before KeyFrame::ComputeBoW
// has filled its FeatureVector (ref: src/KeyFrame.cc:392-400).  So a resident set is a hit only if its feature count, its
// FeatureVector size and its fingerprint (first keypoint, first and last descriptor) are those of the object in hand; otherwise
// it is put again -- from the device block of `builder` when that context has just built this very frame (only the
// FeatureVector travels), from the host otherwise.
template <class T>
bool ensure_set(orbhip_ctx *c, uint64_t key, const T &t, const std::vector<cv::KeyPoint> &keysUn, float minX, float minY, float invW,
                float invH, orbhip_ctx *builder)
{
    const int n = t.mDescriptors.rows;
    if (n <= 0 || (int)keysUn.size() != n) return false;
    const uint64_t fp = orbhip_set_fingerprint_rows(reinterpret_cast<const orbhip_keypoint *>(keysUn.data()), t.mDescriptors.ptr(0),
                                                    t.mDescriptors.ptr(n - 1), n);
    int n0 = 0, ng0 = 0;
    uint64_t fp0 = 0;
    if (orbhip_set_info(c, key, &n0, &ng0, &fp0) && n0 == n && fp0 == fp && ng0 == (int)t.mFeatVec.size()) return true;
    const Csr fv = flatten(t.mFeatVec);
    // the frame its extractor built last is still on the device: block to block, the FeatureVector alone travels
    if (builder && orbhip_frame_fingerprint(builder) == fp &&
        orbhip_set_put_from_frame(c, key, builder, fv.node.data(), fv.off.data(), fv.idx.data(), (int)fv.node.size()) == ORBHIP_OK)
        return true;
    const std::vector<uint8_t> d = contiguous(t.mDescriptors);
    return orbhip_set_put(c, key, reinterpret_cast<const orbhip_keypoint *>(keysUn.data()), d.data(), n, fv.node.data(),
                          fv.off.data(), fv.idx.data(), (int)fv.node.size(), minX, minY, invW, invH) == ORBHIP_OK;
}

// d = R * x + t for 3x3 / 3x1 float matrices.  OpenCV evaluates the MatExpr Rcw*x3Dw+tcw as one gemm whose
// float kernel accumulates in double and rounds once (modules/core/src/matmul.cpp, GEMMSingleMul<float,double>).
inline void affine3(const cv::Mat &R, const float x[3], const float t[3], float out[3], bool transpose = false, double alpha = 1.0)
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)(transpose ? R.at<float>(k, r) : R.at<float>(r, k)) * (double)x[k];
        out[r] = (float)(alpha * s + (t ? (double)t[r] : 0.0));
    }
}

// out = float(alpha * R) (or R transposed): what OpenCV materialises for s*R, R/s and (1/s)*R.t()
inline void scale3(const cv::Mat &R, double alpha, bool transpose, cv::Mat &out)
{
    out = cv::Mat(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++)
            out.at<float>(r, k) = (float)(alpha * (double)(transpose ? R.at<float>(k, r) : R.at<float>(r, k)));
}

// Scw -> Rcw, tcw, Ow (ref: :299-303, :989-993)
inline void decompose_sim3(const cv::Mat &Scw, cv::Mat &Rcw, float tcw[3], float Ow[3])
{
    double dot = 0;
    for (int k = 0; k < 3; k++) dot += (double)Scw.at<float>(0, k) * (double)Scw.at<float>(0, k);
    const float scw = std::sqrt(dot);
    const cv::Mat sRcw = Scw.rowRange(0,3).colRange(0,3);
    scale3(sRcw, 1.0 / scw, false, Rcw);
    for (int r = 0; r < 3; r++) tcw[r] = (float)((double)Scw.at<float>(r, 3) * (1.0 / scw));
    affine3(Rcw, tcw, NULL, Ow, true, -1.0);                   // Ow = -Rcw.t()*tcw
}

// Epipole of key frame 1 in the image of key frame 2 (ref: src/ORBmatcher.cc:664-671): C2 = R2w*Cw+t2w projected
inline void epipole_in_second(KeyFrame *pKF1, KeyFrame *pKF2, float &ex, float &ey)
{
    const cv::Mat Cw(pKF1->GetCameraCenter()), R2w(pKF2->GetRotation()), t2w(pKF2->GetTranslation());
    const float cw[3] = {Cw.at<float>(0, 0), Cw.at<float>(1, 0), Cw.at<float>(2, 0)};
    const float t2[3] = {t2w.at<float>(0, 0), t2w.at<float>(1, 0), t2w.at<float>(2, 0)};
    float C2[3];
    affine3(R2w, cw, t2, C2);                                  // C2 = R2w*Cw+t2w
    const float invz = 1.0f/C2[2];
    ex =pKF2->fx*C2[0]*invz+pKF2->cx;
    ey =pKF2->fy*C2[1]*invz+pKF2->cy;
}

}  // namespace hipdetail
}  // namespace ORB_SLAM2

#endif
