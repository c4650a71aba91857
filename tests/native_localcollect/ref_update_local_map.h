// ref_update_local_map.h -- host restatement of Tracking::UpdateLocalMap (ref: src/Tracking.cc:2407-2562 UpdateLocalKeyFrames
// with mbMonoVIEnable false, :2377-2400 UpdateLocalPoints) on slamlite's KeyFrame / MapPoint / Frame objects, with
// keyframeCounter and the children walked in ascending mnId order (the canonical order of docs/parity.md; the reference walks
// both by heap address).  Shared by tests/native_localcollect/test_localcollect.cpp (the oracle) and
// tools/native/localcollect_latency.cpp (the host side of the measurement).
#ifndef REF_UPDATE_LOCAL_MAP_H
#define REF_UPDATE_LOCAL_MAP_H

#include <map>
#include <set>
#include <vector>

#include "slamlite.h"

namespace refrestate
{
using namespace ORB_SLAM2;

struct ById {
    bool operator()(KeyFrame *a, KeyFrame *b) const { return a->mnId < b->mnId; }
};

// UpdateLocalKeyFrames: the vote, then the covisibility step
static inline void ref_update_key_frames(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, KeyFrame *&pRef)
{
    std::map<KeyFrame *, int, ById> keyframeCounter;
    for (int i = 0; i < F.N; i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (!pMP->isBad()) {
            const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
            for (std::map<KeyFrame *, size_t>::const_iterator it = observations.begin(); it != observations.end(); it++) keyframeCounter[it->first]++;
        } else
            F.mvpMapPoints[i] = NULL;
    }
    if (!keyframeCounter.empty()) {
        int max = 0;
        KeyFrame *pKFmax = NULL;
        vpLocalKeyFrames.clear();
        vpLocalKeyFrames.reserve(3 * keyframeCounter.size());
        for (std::map<KeyFrame *, int, ById>::const_iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); it++) {
            KeyFrame *pKF = it->first;
            if (pKF->isBad()) continue;
            if (it->second > max) max = it->second, pKFmax = pKF;
            vpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = F.mnId;
        }
        for (std::vector<KeyFrame *>::const_iterator itKF = vpLocalKeyFrames.begin(), itEndKF = vpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
            if (vpLocalKeyFrames.size() > 80) break;
            KeyFrame *pKF = *itKF;
            const std::vector<KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vNeighs.size(); k++)
                if (!vNeighs[k]->isBad() && vNeighs[k]->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(vNeighs[k]);
                    vNeighs[k]->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            const std::set<KeyFrame *> sp = pKF->GetChilds();
            const std::set<KeyFrame *, ById> spChilds(sp.begin(), sp.end());
            for (std::set<KeyFrame *, ById>::const_iterator sit = spChilds.begin(); sit != spChilds.end(); sit++)
                if (!(*sit)->isBad() && (*sit)->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(*sit);
                    (*sit)->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            KeyFrame *pParent = pKF->GetParent();
            if (pParent && pParent->mnTrackReferenceForFrame != F.mnId) {
                vpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = F.mnId;
                break;
            }
        }
        if (pKFmax) pRef = pKFmax;
    }
}

// UpdateLocalPoints
static inline void ref_update_points(Frame &F, const std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints)
{
    vpLocalMapPoints.clear();
    for (size_t k = 0; k < vpLocalKeyFrames.size(); k++) {
        const std::vector<MapPoint *> vpMPs = vpLocalKeyFrames[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMPs.size(); i++) {
            MapPoint *pMP = vpMPs[i];
            if (!pMP || pMP->mnTrackReferenceForFrame == F.mnId) continue;
            if (!pMP->isBad()) {
                vpLocalMapPoints.push_back(pMP);
                pMP->mnTrackReferenceForFrame = F.mnId;
            }
        }
    }
}

static inline void ref_update(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints, KeyFrame *&pRef)
{
    ref_update_key_frames(F, vpLocalKeyFrames, pRef);
    ref_update_points(F, vpLocalKeyFrames, vpLocalMapPoints);
}
}  // namespace refrestate

#endif
