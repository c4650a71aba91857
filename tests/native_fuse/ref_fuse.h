// ref_fuse.h -- ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) (ref: src/ORBmatcher.cc:825-975) and the
// two loops of LocalMapping::SearchInNeighbors around it (ref: src/LocalMapping.cc:2549-2581) restated on the host (test
// infrastructure, like oracle/): the C++ twin of tests/fuse_model.py.  The projection is written from the cited lines; the window
// search of one point is the oracle's (oracle/orb_oracle.c, orbo_window_best).  Used by the mock of the entry points
// (mock_fuse.cc, on the store's copies of the points), by the reference side of the mock program (on the MapPoint objects
// themselves, point by point as the reference runs) and by tools/native/fuse_latency.cpp (the host loop on one core).  Compile with
// -ffp-contract=off.
#ifndef ORBHIP_TESTS_REF_FUSE_H
#define ORBHIP_TESTS_REF_FUSE_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "LocalMap.h"
extern "C" {
#include "orb_oracle.h"
}

namespace reffuse
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

inline Camera camera_of(KeyFrame *pKF, float th)
{
    Camera C;
    memset(&C, 0, sizeof C);
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) C.R[3 * r + c] = R.at<float>(r, c);
        C.t[r] = t.at<float>(r, 0), C.Ow[r] = O.at<float>(r, 0);
    }
    C.fx = pKF->fx, C.fy = pKF->fy, C.cx = pKF->cx, C.cy = pKF->cy, C.mbf = pKF->mbf;
    C.minX = pKF->mnMinX, C.maxX = pKF->mnMaxX, C.minY = pKF->mnMinY, C.maxY = pKF->mnMaxY;
    C.nlevels = pKF->mnScaleLevels;
    for (int l = 0; l < C.nlevels && l < 16; l++) C.sf[l] = pKF->mvScaleFactors[l];
    C.logS = pKF->mfLogScaleFactor;
    C.th = th;
    return C;
}

// ref: :850-890.  false where the reference's loop says continue (and for dist3D == 0 or a non-finite ratio: outside the contract)
inline bool fuse_query(const Camera &C, const float xw[3], const float nrm[3], float minDist, float maxDist, orbo_proj_query *q)
{
    memset(q, 0, sizeof *q);
    float pc[3];
    gemm3(C.R, xw, C.t, pc);
    if (pc[2] < 0.0f) return false;
    const float invz = 1 / pc[2];
    const float x = pc[0] * invz;
    const float y = pc[1] * invz;
    const float u = C.fx * x + C.cx;
    const float v = C.fy * y + C.cy;
    if (!(u >= C.minX && u < C.maxX && v >= C.minY && v < C.maxY)) return false;      // KeyFrame::IsInImage
    const float ur = u - C.mbf * invz;
    double sq = 0, dot = 0;
    for (int k = 0; k < 3; k++) {
        const float po = xw[k] - C.Ow[k];
        sq += (double)po * (double)po;
        dot += (double)po * (double)nrm[k];
    }
    const float dist = (float)std::sqrt(sq);
    if (!(dist > 0) || !std::isfinite(dist)) return false;
    if (dist < 0.8f * minDist || dist > 1.2f * maxDist) return false;
    if (dot < 0.5 * dist) return false;
    const float ratio = maxDist / dist;
    if (!std::isfinite(ratio)) return false;
    int level = (int)std::ceil(std::log(ratio) / C.logS);          // MapPoint::PredictScale, ref: src/MapPoint.cc:400-415
    if (level < 0) level = 0;
    else if (level >= C.nlevels) level = C.nlevels - 1;
    q->u = u, q->v = v;
    q->radius = C.th * C.sf[level];
    q->proj_xr = ur;
    q->min_level = level - 1, q->max_level = level;
    q->flags = ORBO_Q_ACTIVE | ORBO_Q_OBSERVED;
    return true;
}

// a key frame's features as the oracle's window search takes them
struct Features {
    std::vector<uint8_t> desc;
    const orbo_keypoint *kps;
    const float *uRight, *sigma;
    int n;
    float gp[4];
};
inline Features features_of(KeyFrame *pKF)
{
    Features F;
    F.n = (int)pKF->mvKeysUn.size();
    F.desc.resize((size_t)F.n * 32);
    for (int i = 0; i < F.n; i++) memcpy(&F.desc[(size_t)i * 32], pKF->mDescriptors.ptr(i), 32);
    F.kps = reinterpret_cast<const orbo_keypoint *>(pKF->mvKeysUn.data());
    F.uRight = (int)pKF->mvuRight.size() == F.n ? pKF->mvuRight.data() : NULL;
    F.sigma = pKF->mvInvLevelSigma2.data();
    F.gp[0] = pKF->mnMinX, F.gp[1] = pKF->mnMinY, F.gp[2] = pKF->mfGridElementWidthInv, F.gp[3] = pKF->mfGridElementHeightInv;
    return F;
}
inline void best_of(const Features &F, const orbo_proj_query &q, const uint8_t *qdesc, int32_t *bi, int32_t *bd)
{
    orbo_window_best(F.kps, F.desc.data(), F.n, F.uRight, F.sigma, F.gp[0], F.gp[1], F.gp[2], F.gp[3], &q, qdesc, 1, bi, bd);
}

// what the scene must contain for the rule about changed descriptors to be tested at all (the mock program asserts it)
struct Stats {
    std::map<MapPoint *, std::vector<uint8_t> > first;   // every source point's descriptor when the pass began
    long changedActive = 0, changedDiffers = 0, replaced = 0, added = 0;
};

// the reference's Fuse, point by point: a point's descriptor is read when its turn comes
inline int Fuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMapPoints, float th, Stats *st = NULL)
{
    const Camera C = camera_of(pKF, th);
    const Features F = features_of(pKF);
    int nFused = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
        MapPoint *pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const cv::Mat P = pMP->GetWorldPos(), N = pMP->GetNormal();
        const float xw[3] = {P.at<float>(0, 0), P.at<float>(1, 0), P.at<float>(2, 0)};
        const float nrm[3] = {N.at<float>(0, 0), N.at<float>(1, 0), N.at<float>(2, 0)};
        orbo_proj_query q;
        if (!fuse_query(C, xw, nrm, pMP->mfMinDistance, pMP->mfMaxDistance, &q)) continue;
        const cv::Mat dMP = pMP->GetDescriptor();
        int32_t bestIdx = -1, bestDist = 256;
        best_of(F, q, dMP.ptr(0), &bestIdx, &bestDist);
        if (st && st->first.count(pMP) && memcmp(st->first[pMP].data(), dMP.ptr(0), 32) != 0) {
            int32_t oi = -1, od = 256;
            best_of(F, q, st->first[pMP].data(), &oi, &od);
            st->changedActive++;
            if (oi != bestIdx && (od <= 50 || bestDist <= 50)) st->changedDiffers++;
        }
        if (bestDist <= 50) {                                          // TH_LOW
            MapPoint *pMPinKF = pKF->GetMapPoint(bestIdx);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                    if (st) st->replaced++;
                }
            } else {
                pMP->AddObservation(pKF, bestIdx);
                pKF->AddMapPoint(pMP, bestIdx);
                if (st) st->added++;
            }
            nFused++;
        }
    }
    return nFused;
}

// ref: src/LocalMapping.cc:2549-2556
inline std::vector<int> FuseInTargets(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th, Stats *st = NULL)
{
    const std::vector<MapPoint *> vpMapPointMatches = pKF->GetMapPointMatches();
    if (st)
        for (size_t i = 0; i < vpMapPointMatches.size(); i++)
            if (vpMapPointMatches[i]) {
                const cv::Mat d = vpMapPointMatches[i]->GetDescriptor();
                st->first[vpMapPointMatches[i]].assign(d.ptr(0), d.ptr(0) + 32);
            }
    std::vector<int> n;
    for (size_t k = 0; k < vpTargetKFs.size(); k++) n.push_back(Fuse(vpTargetKFs[k], vpMapPointMatches, th, st));
    return n;
}

// ref: :2558-2581 (the stamp mnFuseCandidateForKF is a set here)
inline std::vector<MapPoint *> Candidates(const std::vector<KeyFrame *> &vpTargetKFs)
{
    std::vector<MapPoint *> vpFuseCandidates;
    std::set<MapPoint *> stamped;
    for (size_t k = 0; k < vpTargetKFs.size(); k++) {
        const std::vector<MapPoint *> vp = vpTargetKFs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vp.size(); i++) {
            MapPoint *pMP = vp[i];
            if (!pMP) continue;
            if (pMP->isBad() || stamped.count(pMP)) continue;
            stamped.insert(pMP);
            vpFuseCandidates.push_back(pMP);
        }
    }
    return vpFuseCandidates;
}
inline int FuseCandidates(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th)
{
    return Fuse(pKF, Candidates(vpTargetKFs), th);
}
}  // namespace reffuse

#endif
