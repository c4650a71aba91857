// ref_sim3.h -- ORBmatcher::SearchBySim3 (ref: src/ORBmatcher.cc:1102-1326) restated on the host (test infrastructure, like oracle/):
// the C++ twin of tests/sim3search_model.py.  The projection is written from the cited lines; the window search of one point is
// the oracle's without a gate (oracle/orb_oracle.c, orbo_window_best).  Used by the mock of the entry point (mock_sim3search.cc, on
// the store's copies of the points), by the reference side of the mock program (on the MapPoint objects themselves) and by
// tools/native/sim3search_latency.cpp.  Compile with -ffp-contract=off.
#ifndef ORBHIP_TESTS_REF_SIM3_H
#define ORBHIP_TESTS_REF_SIM3_H

#include "ref_fuse.h"

namespace refsim3
{
using namespace ORB_SLAM2;
using reffuse::Camera;
using reffuse::gemm3;

// sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (:1119-1121): the double factor times the float entry, rounded once
struct Sim3 {
    float sR12[9], sR21[9], t12[3], t21[3];
};
inline Sim3 compose(float s12, const cv::Mat &R12, const cv::Mat &t12)
{
    Sim3 S;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            S.sR12[3 * r + c] = (float)((double)s12 * (double)R12.at<float>(r, c));
            S.sR21[3 * r + c] = (float)((1.0 / s12) * (double)R12.at<float>(c, r));
        }
    for (int r = 0; r < 3; r++) S.t12[r] = t12.at<float>(r, 0);
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)S.sR21[3 * r + k] * (double)S.t12[k];
        S.t21[r] = (float)(-1.0 * s + 0.0);
    }
    return S;
}

// :1158-1189 (or :1238-1269).  src: the source key frame's pose; sR, t: into the destination camera; K1: key frame 1 (fx, fy, cx,
// cy -- in both directions); dst: bounds and scale tables.  false where the loop says continue (and for dist3D == 0 or a non-finite
// ratio: outside the contract)
inline bool sim3_query(const Camera &src, const float sR[9], const float t[3], const Camera &K1, const Camera &dst, float th,
                       const float xw[3], float minDist, float maxDist, orbo_proj_query *q)
{
    memset(q, 0, sizeof *q);
    float p1[3], p2[3];
    gemm3(src.R, xw, src.t, p1);
    gemm3(sR, p1, t, p2);
    if (p2[2] < 0.0) return false;
    const float invz = 1.0 / p2[2];
    const float x = p2[0] * invz;
    const float y = p2[1] * invz;
    const float u = K1.fx * x + K1.cx;
    const float v = K1.fy * y + K1.cy;
    if (!(u >= dst.minX && u < dst.maxX && v >= dst.minY && v < dst.maxY)) return false;      // KeyFrame::IsInImage
    double sq = 0;
    for (int k = 0; k < 3; k++) sq += (double)p2[k] * (double)p2[k];
    const float dist = (float)std::sqrt(sq);                                               // cv::norm of the camera point
    if (!(dist > 0) || !std::isfinite(dist)) return false;
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) return false;
    const float ratio = maxDist / dist;
    if (!std::isfinite(ratio)) return false;
    int level = (int)std::ceil(std::log(ratio) / dst.logS);                                 // MapPoint::PredictScale
    if (level < 0) level = 0;
    else if (level >= dst.nlevels) level = dst.nlevels - 1;
    q->u = u, q->v = v;
    q->radius = th * dst.sf[level];
    q->min_level = level - 1, q->max_level = level;
    q->flags = ORBO_Q_ACTIVE | ORBO_Q_OBSERVED;
    return true;
}

// :1221, :1301, :1310-1323 over the two tables; match12 [n1]
inline int agree(const std::vector<int32_t> &best1, const std::vector<int32_t> &dist1, const std::vector<int32_t> &best2,
                 const std::vector<int32_t> &dist2, int thHigh, std::vector<int32_t> &match12)
{
    const int n1 = (int)best1.size(), n2 = (int)best2.size();
    match12.assign(n1, -1);
    int found = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        const int i2 = dist1[i1] <= thHigh ? best1[i1] : -1;
        if (i2 < 0 || i2 >= n2) continue;
        if ((dist2[i2] <= thHigh ? best2[i2] : -1) == i1) match12[i1] = i2, found++;
    }
    return found;
}

struct Stats {
    int oneSided0 = 0, oneSided1 = 0, active0 = 0, active1 = 0;
};

// the reference on the objects: the same return value and edits to vpMatches12
inline int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, float s12, const cv::Mat &R12, const cv::Mat &t12,
                        float th, Stats *st = NULL)
{
    const Sim3 S = compose(s12, R12, t12);
    KeyFrame *kf[2] = {pKF1, pKF2};
    const Camera cam[2] = {reffuse::camera_of(pKF1, th), reffuse::camera_of(pKF2, th)};
    const std::vector<MapPoint *> pts[2] = {pKF1->GetMapPointMatches(), pKF2->GetMapPointMatches()};
    const int N[2] = {(int)pts[0].size(), (int)pts[1].size()};
    std::vector<bool> taken[2] = {std::vector<bool>(N[0], false), std::vector<bool>(N[1], false)};
    for (int i = 0; i < N[0]; i++) {
        MapPoint *pMP = vpMatches12[i];
        if (!pMP) continue;
        taken[0][i] = true;
        const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
        if (idx2 >= 0 && idx2 < N[1]) taken[1][idx2] = true;
    }
    std::vector<int32_t> best[2], dist[2];
    for (int d = 0; d < 2; d++) {
        const reffuse::Features F = reffuse::features_of(kf[1 - d]);
        best[d].assign(N[d], -1), dist[d].assign(N[d], 256);
        for (int i = 0; i < N[d]; i++) {
            MapPoint *pMP = pts[d][i];
            if (!pMP || taken[d][i]) continue;
            if (pMP->isBad()) continue;
            const cv::Mat P = pMP->GetWorldPos();
            const float xw[3] = {P.at<float>(0, 0), P.at<float>(1, 0), P.at<float>(2, 0)};
            orbo_proj_query q;
            if (!sim3_query(cam[d], d == 0 ? S.sR21 : S.sR12, d == 0 ? S.t21 : S.t12, cam[0], cam[1 - d], th, xw, pMP->mfMinDistance,
                            pMP->mfMaxDistance, &q))
                continue;
            if (st) (d == 0 ? st->active0 : st->active1)++;
            const cv::Mat dMP = pMP->GetDescriptor();
            orbo_window_best(F.kps, F.desc.data(), F.n, NULL, NULL, F.gp[0], F.gp[1], F.gp[2], F.gp[3], &q, dMP.ptr(0), 1, &best[d][i], &dist[d][i]);
        }
    }
    std::vector<int32_t> match12;
    const int found = agree(best[0], dist[0], best[1], dist[1], 100, match12);
    for (int i1 = 0; i1 < N[0]; i1++)
        if (match12[i1] >= 0) vpMatches12[i1] = pts[1][match12[i1]];
    if (st) {
        for (int i1 = 0; i1 < N[0]; i1++)
            if (dist[0][i1] <= 100 && best[0][i1] >= 0 && match12[i1] < 0) st->oneSided0++;
        for (int i2 = 0; i2 < N[1]; i2++)
            if (dist[1][i2] <= 100 && best[1][i2] >= 0 && (match12[best[1][i2]] != i2)) st->oneSided1++;
    }
    return found;
}
}  // namespace refsim3

#endif
