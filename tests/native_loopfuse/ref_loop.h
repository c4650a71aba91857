// ref_loop.h -- LoopClosing's two projection searches restated on the host from the cited lines (test infrastructure, like
// oracle/): ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, vpPoints, vpMatched, th) (ref: src/ORBmatcher.cc:290-403),
// ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (ref: :977-1100), the union of LoopClosing::ComputeSim3
// (ref: src/LoopClosing.cc:404-424) and LoopClosing::SearchAndFuse (ref: :647-673).  The C++ twin of tests/loopfuse_model.py: the
// projection of one point is that of Fuse(pKF, vpMapPoints, th) line for line and is taken from tests/native_fuse/ref_fuse.h; the
// decomposition of the similarity, "already found" as a set of points, the window search without a gate and the sequential claim
// are written out here.  Used by the mock of the entry points (mock_loopfuse.cc, on the store's copies of the points) and by the
// reference side of the mock program (on the MapPoint objects themselves, point by point as the reference runs).  Compile with
// -ffp-contract=off.
#ifndef ORBHIP_TESTS_REF_LOOP_H
#define ORBHIP_TESTS_REF_LOOP_H

#include <utility>

#include "ref_fuse.h"

namespace refloop
{
using namespace ORB_SLAM2;
using reffuse::Camera;
using reffuse::Features;

// ref: src/ORBmatcher.cc:299-303, :986-990.  sqrt of a double dot product, rounded to float; sRcw / scw and t / scw are products
// with the double 1 / scw, rounded once; Ow = -Rcw' tcw is one gemm
inline void decompose(const cv::Mat &Scw, float R[9], float t[3], float Ow[3])
{
    double dot = 0;
    for (int k = 0; k < 3; k++) dot += (double)Scw.at<float>(0, k) * (double)Scw.at<float>(0, k);
    const float scw = (float)std::sqrt(dot);
    const double inv = 1.0 / (double)scw;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[3 * r + c] = (float)((double)Scw.at<float>(r, c) * inv);
        t[r] = (float)((double)Scw.at<float>(r, 3) * inv);
    }
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)R[3 * k + r] * (double)t[k];
        Ow[r] = (float)(-1.0 * s);
    }
}

inline Camera camera_of(KeyFrame *pKF, const cv::Mat &Scw, float th)
{
    Camera C = reffuse::camera_of(pKF, th);
    decompose(Scw, C.R, C.t, C.Ow);
    return C;
}

// :320-360 and :1008-1049: the projection of Fuse; there is no right coordinate
inline bool sim3_query(const Camera &C, MapPoint *pMP, orbo_proj_query *q)
{
    const cv::Mat P = pMP->GetWorldPos(), N = pMP->GetNormal();
    const float xw[3] = {P.at<float>(0, 0), P.at<float>(1, 0), P.at<float>(2, 0)};
    const float nrm[3] = {N.at<float>(0, 0), N.at<float>(1, 0), N.at<float>(2, 0)};
    const bool in = reffuse::fuse_query(C, xw, nrm, pMP->mfMinDistance, pMP->mfMaxDistance, q);
    q->proj_xr = 0;
    return in;
}

// :1051-1079: no chi-square test
inline void best_ungated(const Features &F, const orbo_proj_query &q, const uint8_t *qdesc, int32_t *bi, int32_t *bd)
{
    orbo_window_best(F.kps, F.desc.data(), F.n, NULL, NULL, F.gp[0], F.gp[1], F.gp[2], F.gp[3], &q, qdesc, 1, bi, bd);
}

inline int hamming(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

// what the scene must contain for the sequencing rules to be tested at all (the mock program asserts it)
struct Stats {
    std::map<MapPoint *, std::vector<uint8_t> > first;          // every loop point's descriptor when SearchAndFuse began
    std::set<std::pair<KeyFrame *, MapPoint *> > heldAtStart;   // (target, loop point) pairs that were held then
    long changedActive = 0, changedDiffers = 0, heldLater = 0, addedThenHeld = 0, replaced = 0, added = 0;
};

// ref: src/ORBmatcher.cc:977-1100, point by point: a point's descriptor is read when its turn comes
inline int Fuse(KeyFrame *pKF, const cv::Mat &Scw, const std::vector<MapPoint *> &vpPoints, float th, std::vector<MapPoint *> &vpReplacePoint,
                Stats *st = NULL)
{
    const Camera C = camera_of(pKF, Scw, th);
    const Features F = reffuse::features_of(pKF);
    const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();
    std::set<MapPoint *> addedHere;
    int nFused = 0;
    for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
        MapPoint *pMP = vpPoints[iMP];
        if (pMP->isBad()) continue;
        if (spAlreadyFound.count(pMP)) {
            if (st && !st->heldAtStart.count(std::make_pair(pKF, pMP))) st->heldLater++;
            continue;
        }
        orbo_proj_query q;
        if (!sim3_query(C, pMP, &q)) continue;
        const cv::Mat dMP = pMP->GetDescriptor();
        int32_t bestIdx = -1, bestDist = 256;
        best_ungated(F, q, dMP.ptr(0), &bestIdx, &bestDist);
        if (st && st->first.count(pMP) && memcmp(st->first[pMP].data(), dMP.ptr(0), 32) != 0) {
            int32_t oi = -1, od = 256;
            best_ungated(F, q, st->first[pMP].data(), &oi, &od);
            st->changedActive++;
            if (oi != bestIdx && (od <= 50 || bestDist <= 50)) st->changedDiffers++;
        }
        if (bestDist <= 50) {                                          // TH_LOW
            MapPoint *pMPinKF = pKF->GetMapPoint(bestIdx);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    vpReplacePoint[iMP] = pMPinKF;
                    if (st && addedHere.count(pMPinKF)) st->addedThenHeld++;
                }
            } else {
                pMP->AddObservation(pKF, bestIdx);
                pKF->AddMapPoint(pMP, bestIdx);
                addedHere.insert(pMP);
                if (st) st->added++;
            }
            nFused++;
        }
    }
    return nFused;
}

// ref: src/LoopClosing.cc:647-673, in the order of the vector
inline void SearchAndFuse(const std::vector<std::pair<KeyFrame *, cv::Mat> > &vCorrectedPoses, const std::vector<MapPoint *> &vpLoopMapPoints,
                          float th, Stats *st = NULL)
{
    if (st) {
        for (size_t i = 0; i < vpLoopMapPoints.size(); i++) {
            const cv::Mat d = vpLoopMapPoints[i]->GetDescriptor();
            st->first[vpLoopMapPoints[i]].assign(d.ptr(0), d.ptr(0) + 32);
            for (size_t k = 0; k < vCorrectedPoses.size(); k++)
                if (vpLoopMapPoints[i]->IsInKeyFrame(vCorrectedPoses[k].first))
                    st->heldAtStart.insert(std::make_pair(vCorrectedPoses[k].first, vpLoopMapPoints[i]));
        }
    }
    for (size_t k = 0; k < vCorrectedPoses.size(); k++) {
        KeyFrame *pKF = vCorrectedPoses[k].first;
        std::vector<MapPoint *> vpReplacePoints(vpLoopMapPoints.size(), static_cast<MapPoint *>(NULL));
        Fuse(pKF, vCorrectedPoses[k].second, vpLoopMapPoints, th, vpReplacePoints, st);
        const int nLP = (int)vpLoopMapPoints.size();
        for (int i = 0; i < nLP; i++) {
            MapPoint *pRep = vpReplacePoints[i];
            if (pRep) {
                pRep->Replace(vpLoopMapPoints[i]);
                if (st) st->replaced++;
            }
        }
    }
}

// ref: src/LoopClosing.cc:404-424 (the stamp mnLoopPointForKF is a set here)
inline std::vector<MapPoint *> LoopPoints(const std::vector<KeyFrame *> &vpLoopConnectedKFs)
{
    std::vector<MapPoint *> vpLoopMapPoints;
    std::set<MapPoint *> stamped;
    for (size_t k = 0; k < vpLoopConnectedKFs.size(); k++) {
        const std::vector<MapPoint *> vpMapPoints = vpLoopConnectedKFs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPoints.size(); i++) {
            MapPoint *pMP = vpMapPoints[i];
            if (pMP && !pMP->isBad() && !stamped.count(pMP)) {
                vpLoopMapPoints.push_back(pMP);
                stamped.insert(pMP);
            }
        }
    }
    return vpLoopMapPoints;
}

// ref: src/ORBmatcher.cc:290-403, point by point
inline int SearchByProjection(KeyFrame *pKF, const cv::Mat &Scw, const std::vector<MapPoint *> &vpPoints, std::vector<MapPoint *> &vpMatched, int th)
{
    const Camera C = camera_of(pKF, Scw, (float)th);
    const Features F = reffuse::features_of(pKF);
    std::vector<int32_t> cellOff(64 * 48 + 1), cellIdx(F.n > 0 ? F.n : 1), area(F.n > 0 ? F.n : 1);
    orbo_grid_build(F.kps, F.n, F.gp[0], F.gp[1], F.gp[2], F.gp[3], cellOff.data(), cellIdx.data());
    std::set<MapPoint *> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPoint *>(NULL));
    int nmatches = 0;
    for (size_t iMP = 0; iMP < vpPoints.size(); iMP++) {
        MapPoint *pMP = vpPoints[iMP];
        if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        orbo_proj_query q;
        if (!sim3_query(C, pMP, &q)) continue;
        const int nIdx = orbo_features_in_area(F.kps, cellOff.data(), cellIdx.data(), F.gp[0], F.gp[1], F.gp[2], F.gp[3], q.u, q.v, q.radius, -1,
                                               -1, area.data(), (int)area.size());
        if (nIdx == 0) continue;
        const cv::Mat dMP = pMP->GetDescriptor();
        int bestDist = 256, bestIdx = -1;
        for (int k = 0; k < nIdx; k++) {
            const int idx = area[k];
            if (vpMatched[idx]) continue;
            const int kpLevel = F.kps[idx].octave;
            if (kpLevel < q.min_level || kpLevel > q.max_level) continue;
            const int dist = hamming(dMP.ptr(0), &F.desc[(size_t)idx * 32]);
            if (dist < bestDist) bestDist = dist, bestIdx = idx;
        }
        if (bestDist <= 50) {                                          // TH_LOW
            vpMatched[bestIdx] = pMP;
            nmatches++;
        }
    }
    return nmatches;
}
}  // namespace refloop

#endif
