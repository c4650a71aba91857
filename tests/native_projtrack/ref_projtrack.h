// ref_projtrack.h -- the two projection loops of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ref:
// src/ORBmatcher.cc:1341-1498) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ref: :1500-1627) restated
// on the host (test infrastructure, like oracle/): the C++ twin of tests/projtrack_model.py.  The loops make the queries; the
// window search behind them is the oracle's (oracle/orb_oracle.c).  Used by the mock of the entry points (mock_projtrack.cc,
// on the store's copies of the points), by the reference side of the mock program (on the MapPoint objects themselves) and by
// tools/native/projtrack_latency.cpp (the host loop on one core).  Compile with -ffp-contract=off.
#ifndef ORBHIP_TESTS_REF_PROJTRACK_H
#define ORBHIP_TESTS_REF_PROJTRACK_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <set>
#include <vector>

#include "LocalMap.h"
extern "C" {
#include "orb_oracle.h"
}

namespace refpt
{
using namespace ORB_SLAM2;

struct Camera {
    float R[9], t[3], Ow[3], fx, fy, cx, cy, mbf, minX, maxX, minY, maxY, sf[16], logS, th;
    int nlevels;
};

// one gemm: products and sums in double, one rounding (OpenCV's GEMMSingleMul<float,double>)
inline void gemm3(const float R[9], const float x[3], const float t[3], float out[3])
{
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)R[3 * r + k] * (double)x[k];
        out[r] = (float)(s + (double)t[r]);
    }
}

inline Camera camera_of(const Frame &F, float th)
{
    Camera C;
    memset(&C, 0, sizeof C);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) C.R[3 * r + c] = F.mTcw.at<float>(r, c);
        C.t[r] = F.mTcw.at<float>(r, 3);
    }
    for (int r = 0; r < 3; r++) {   // -R' t
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)C.R[3 * k + r] * (double)C.t[k];
        C.Ow[r] = (float)(-1.0 * s);
    }
    C.fx = Frame::fx, C.fy = Frame::fy, C.cx = Frame::cx, C.cy = Frame::cy, C.mbf = F.mbf;
    C.minX = Frame::mnMinX, C.maxX = Frame::mnMaxX, C.minY = Frame::mnMinY, C.maxY = Frame::mnMaxY;
    C.nlevels = F.mnScaleLevels;
    for (int l = 0; l < C.nlevels && l < 16; l++) C.sf[l] = F.mvScaleFactors[l];
    C.logS = F.mfLogScaleFactor;
    C.th = th;
    return C;
}

// false: outside the image, or outside the contract (a non-finite position, reciprocal depth, u or v)
inline bool project(const Camera &C, const float xw[3], float *u, float *v, float *invz)
{
    if (!std::isfinite(xw[0]) || !std::isfinite(xw[1]) || !std::isfinite(xw[2])) return false;
    float pc[3];
    gemm3(C.R, xw, C.t, pc);
    const float iz = 1.0 / pc[2];                       // ref: :1381, :1530 (a double division)
    if (!std::isfinite(iz)) return false;
    *u = C.fx * pc[0] * iz + C.cx;
    *v = C.fy * pc[1] * iz + C.cy;
    *invz = iz;
    if (!std::isfinite(*u) || !std::isfinite(*v)) return false;
    return !(*u < C.minX || *u > C.maxX || *v < C.minY || *v > C.maxY);
}

// ref: :1376-1416.  motion: 0 same, 1 forward, 2 backward
inline bool last_query(const Camera &C, const float xw[3], bool observed, int octave, float angle, int motion, orbo_proj_query *q)
{
    float u, v, invz;
    memset(q, 0, sizeof *q);
    if (!project(C, xw, &u, &v, &invz) || invz < 0) return false;
    if (octave < 0 || octave >= C.nlevels) return false;
    q->u = u, q->v = v;
    q->radius = C.th * C.sf[octave];
    q->proj_xr = u - C.mbf * invz;
    q->min_level = motion == 1 ? octave : motion == 2 ? 0 : octave - 1;
    q->max_level = motion == 1 ? -1 : motion == 2 ? octave : octave + 1;
    q->angle = angle;
    q->flags = ORBO_Q_ACTIVE | (observed ? ORBO_Q_OBSERVED : 0);
    return true;
}

// ref: :1524-1558 (no depth-sign test)
inline bool kf_query(const Camera &C, const float xw[3], float minDist, float maxDist, float angle, orbo_proj_query *q)
{
    float u, v, invz;
    memset(q, 0, sizeof *q);
    if (!project(C, xw, &u, &v, &invz)) return false;
    double sq = 0;
    for (int k = 0; k < 3; k++) {
        const float po = xw[k] - C.Ow[k];
        sq += (double)po * (double)po;
    }
    const float dist = (float)std::sqrt(sq);
    if (!(dist > 0) || !std::isfinite(dist)) return false;
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) return false;
    const float ratio = maxDist / dist;
    if (!std::isfinite(ratio)) return false;
    int level = (int)std::ceil(std::log(ratio) / C.logS);          // MapPoint::PredictScale, ref: src/MapPoint.cc:417-432
    if (level < 0) level = 0;
    else if (level >= C.nlevels) level = C.nlevels - 1;
    q->u = u, q->v = v;
    q->radius = C.th * C.sf[level];
    q->min_level = level - 1, q->max_level = level + 1;
    q->angle = angle;
    q->flags = ORBO_Q_ACTIVE | ORBO_Q_OBSERVED;
    return true;
}

inline int motion_of(const Frame &Cur, const Frame &Last, bool bMono)
{
    const Camera C = camera_of(Cur, 0), L = camera_of(Last, 0);
    float tlc[3];
    gemm3(L.R, C.Ow, L.t, tlc);                          // ref: :1351-1365
    if (!bMono && tlc[2] > Cur.mb) return 1;
    if (!bMono && -tlc[2] > Cur.mb) return 2;
    return 0;
}

inline void world_pos(MapPoint *p, float xw[3])
{
    const cv::Mat P = p->GetWorldPos();
    for (int k = 0; k < 3; k++) xw[k] = P.at<float>(k, 0);
}

// the window search of the oracle over the frame, and the reference's write-back
inline int window_search(Frame &Cur, const std::vector<orbo_proj_query> &q, const std::vector<uint8_t> &qdesc,
                         const std::vector<MapPoint *> &source, bool anyPointCloses, bool useRight, bool checkOri, int thHigh)
{
    const int n = Cur.N;
    std::vector<uint8_t> occ(n, 0), d((size_t)n * 32);
    for (int i = 0; i < n; i++) {
        if (Cur.mvpMapPoints[i] && (anyPointCloses || Cur.mvpMapPoints[i]->Observations() > 0)) occ[i] = 1;
        memcpy(&d[(size_t)i * 32], Cur.mDescriptors.ptr(i), 32);
    }
    std::vector<int32_t> match(n);
    const int found = orbo_search_by_projection(
        reinterpret_cast<const orbo_keypoint *>(Cur.mvKeysUn.data()), d.data(), n,
        (useRight && (int)Cur.mvuRight.size() == n) ? Cur.mvuRight.data() : NULL, occ.data(), Frame::mnMinX, Frame::mnMinY,
        Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv, q.data(), qdesc.data(), (int)q.size(), 0, 0.f, checkOri ? 1 : 0,
        thHigh, match.data());
    for (int i = 0; i < n; i++) {
        if (match[i] >= 0) Cur.mvpMapPoints[i] = source[match[i]];
        else if (match[i] == -2) Cur.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
    }
    return found;
}

// the two reference routines on the caller's objects
inline int SearchLastFrame(Frame &Cur, const Frame &Last, float th, bool bMono, bool checkOri)
{
    if (Cur.N == 0 || Last.N == 0) return 0;
    const Camera C = camera_of(Cur, th);
    const int motion = motion_of(Cur, Last, bMono);
    std::vector<orbo_proj_query> q(Last.N);
    std::vector<uint8_t> qdesc((size_t)Last.N * 32, 0);
    for (int i = 0; i < Last.N; i++) {
        memset(&q[i], 0, sizeof q[i]);
        MapPoint *p = Last.mvpMapPoints[i];
        if (!p || Last.mvbOutlier[i]) continue;
        float xw[3];
        world_pos(p, xw);
        if (last_query(C, xw, p->Observations() > 0, Last.mvKeys[i].octave, Last.mvKeysUn[i].angle, motion, &q[i]))
            memcpy(&qdesc[(size_t)i * 32], p->GetDescriptor().ptr(0), 32);
    }
    return window_search(Cur, q, qdesc, Last.mvpMapPoints, false, true, checkOri, 100);
}

inline int SearchKeyFramePoints(Frame &Cur, KeyFrame *pKF, const std::set<MapPoint *> &found, float th, int ORBdist, bool checkOri)
{
    const std::vector<MapPoint *> vp = pKF->GetMapPointMatches();
    if (Cur.N == 0 || vp.empty()) return 0;
    const Camera C = camera_of(Cur, th);
    std::vector<orbo_proj_query> q(vp.size());
    std::vector<uint8_t> qdesc(vp.size() * 32, 0);
    for (size_t i = 0; i < vp.size(); i++) {
        memset(&q[i], 0, sizeof q[i]);
        MapPoint *p = vp[i];
        if (!p || p->isBad() || found.count(p)) continue;
        float xw[3];
        world_pos(p, xw);
        if (kf_query(C, xw, p->mfMinDistance, p->mfMaxDistance, pKF->mvKeysUn[i].angle, &q[i]))
            memcpy(&qdesc[i * 32], p->GetDescriptor().ptr(0), 32);
    }
    return window_search(Cur, q, qdesc, vp, true, false, checkOri, ORBdist);
}
}  // namespace refpt

#endif
