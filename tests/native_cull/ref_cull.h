// ref_cull.h -- the sequential loop of LocalMapping::KeyFrameCulling (ref: src/LocalMapping.cc:2692-2756; the fork's
// KeyFrameCullingForMonoVI, :1477-1584, has the same body behind its tests of the local window) on slamlite.h objects: what
// LocalMapSearch::KeyFrameCulling must equal.  Every candidate is counted on the map as the culls before it left it.
#ifndef ORBHIP_TEST_REF_CULL_H
#define ORBHIP_TEST_REF_CULL_H

#include <map>
#include <vector>

#include "slamlite.h"

namespace refcull
{
struct Count {
    int nMPs, nRedundant;
    bool bRedundant;
};

inline Count count(ORB_SLAM2::KeyFrame *pKF, bool bMonocular)
{
    using namespace ORB_SLAM2;
    const std::vector<MapPoint *> vpMapPoints = pKF->GetMapPointMatches();
    const int thObs = 3;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad()) continue;
        if (!bMonocular) {
            if (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0) continue;
        }
        nMPs++;
        if (pMP->Observations() > thObs) {
            const int scaleLevel = pKF->mvKeysUn[i].octave;
            const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
            int nObs = 0;
            for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                KeyFrame *pKFi = mit->first;
                if (pKFi == pKF) continue;
                const int scaleLeveli = pKFi->mvKeysUn[mit->second].octave;
                if (scaleLeveli <= scaleLevel + 1) {
                    nObs++;
                    if (nObs >= thObs) break;
                }
            }
            if (nObs >= thObs) nRedundantObservations++;
        }
    }
    const Count c = {nMPs, nRedundantObservations, nRedundantObservations > 0.9 * nMPs};
    return c;
}

// returns the culled key frames in order
template <class Skip>
std::vector<ORB_SLAM2::KeyFrame *> KeyFrameCulling(const std::vector<ORB_SLAM2::KeyFrame *> &vpLocalKeyFrames, bool bMonocular, Skip skip)
{
    std::vector<ORB_SLAM2::KeyFrame *> culled;
    for (size_t k = 0; k < vpLocalKeyFrames.size(); k++) {
        ORB_SLAM2::KeyFrame *pKF = vpLocalKeyFrames[k];
        if (pKF->mnId == 0) continue;
        if (skip(pKF)) continue;
        if (count(pKF, bMonocular).bRedundant) {
            pKF->SetBadFlag();
            culled.push_back(pKF);
        }
    }
    return culled;
}
}  // namespace refcull

#endif
