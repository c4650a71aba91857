// ref_ba.h -- the three loops Optimizer::LocalBundleAdjustment runs before the solver sees a vertex (ref: src/Optimizer.cc:2772-2784
// the local key frames, :2786-2802 lLocalMapPoints, :2804-2820 lFixedCameras, :2888 ff. the edges) on slamlite.h objects: what
// LocalMapSearch::BuildLocalBA / BuildBAProblem must equal.  Where the reference walks map<KeyFrame*, size_t> by heap address the
// walk here is in ascending mnId (docs/parity.md); where it allocates a g2o edge, (pKF, idx) is pushed.
#ifndef ORBHIP_TEST_REF_BA_H
#define ORBHIP_TEST_REF_BA_H

#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <vector>

#include "slamlite.h"

namespace refba
{
struct Edge {
    ORB_SLAM2::KeyFrame *pKF;
    size_t idx;
};
struct Problem {
    std::vector<ORB_SLAM2::KeyFrame *> vpLocalKFs, vpFixedKFs;
    std::vector<ORB_SLAM2::MapPoint *> vpLocalMPs;
    std::vector<int32_t> vEdgeOff;
    std::vector<Edge> vEdges;
};

inline bool by_id(const std::pair<ORB_SLAM2::KeyFrame *, size_t> &a, const std::pair<ORB_SLAM2::KeyFrame *, size_t> &b)
{
    return a.first->mnId < b.first->mnId;
}

// GetObservations() in the canonical order
inline std::vector<std::pair<ORB_SLAM2::KeyFrame *, size_t> > observations(ORB_SLAM2::MapPoint *pMP)
{
    const std::map<ORB_SLAM2::KeyFrame *, size_t> m = pMP->GetObservations();
    std::vector<std::pair<ORB_SLAM2::KeyFrame *, size_t> > v(m.begin(), m.end());
    std::sort(v.begin(), v.end(), by_id);
    return v;
}

// ref: :2772-2784
inline std::list<ORB_SLAM2::KeyFrame *> LocalKeyFrames(ORB_SLAM2::KeyFrame *pKF)
{
    using namespace ORB_SLAM2;
    std::list<KeyFrame *> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrame *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame *pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    return lLocalKeyFrames;
}

// ref: :2786-2820 and :2888 ff., for local key frames already stamped with nId
inline void Build(const std::list<ORB_SLAM2::KeyFrame *> &lLocalKeyFrames, unsigned long nId, Problem &out)
{
    using namespace ORB_SLAM2;
    out = Problem();
    out.vpLocalKFs.assign(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
    // Local MapPoints seen in Local KeyFrames
    std::list<MapPoint *> lLocalMapPoints;
    for (std::list<KeyFrame *>::const_iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        std::vector<MapPoint *> vpMPs = (*lit)->GetMapPointMatches();
        for (std::vector<MapPoint *>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint *pMP = *vit;
            if (pMP)
                if (!pMP->isBad())
                    if (pMP->mnBALocalForKF != nId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = nId;
                    }
        }
    }
    // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes
    std::list<KeyFrame *> lFixedCameras;
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        const std::vector<std::pair<KeyFrame *, size_t> > obs = observations(*lit);
        for (size_t m = 0; m < obs.size(); m++) {
            KeyFrame *pKFi = obs[m].first;
            if (pKFi->mnBALocalForKF != nId && pKFi->mnBAFixedForKF != nId) {
                pKFi->mnBAFixedForKF = nId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }
    // Set MapPoint vertices and their edges
    out.vEdgeOff.push_back(0);
    for (std::list<MapPoint *>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        const std::vector<std::pair<KeyFrame *, size_t> > obs = observations(*lit);
        for (size_t m = 0; m < obs.size(); m++) {
            KeyFrame *pKFi = obs[m].first;
            if (!pKFi->isBad()) {
                const Edge e = {pKFi, obs[m].second};
                out.vEdges.push_back(e);
            }
        }
        out.vEdgeOff.push_back((int32_t)out.vEdges.size());
    }
    out.vpLocalMPs.assign(lLocalMapPoints.begin(), lLocalMapPoints.end());
    out.vpFixedKFs.assign(lFixedCameras.begin(), lFixedCameras.end());
}
}  // namespace refba

#endif
