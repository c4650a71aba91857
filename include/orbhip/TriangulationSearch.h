// TriangulationSearch.h -- ORB_SLAM2::TriangulationSearch: the ORBmatcher::SearchForTriangulation calls of
// LocalMapping::CreateNewMapPoints (ref: src/LocalMapping.cc:2258-2298, one per neighbour of the new key frame, 20 in the
// monocular case) as ONE device call (orbhip_search_for_triangulation_sets; include/orbhip.h).  No
// counterpart class in the reference: the caller runs its baseline checks and ComputeF12 for all neighbours first, hands the
// neighbours over, and triangulates from the pairs afterwards.  vvMatchedPairs[k] is what
// ORBmatcher(0.6, bCheckOrientation).SearchForTriangulation(pKF1, vpKF2[k], vF12[k], ., bOnlyStereo) fills, in its order
// (ascending index in key frame 1).
//
// Every key frame is kept on the device as a resident set of this object's own context under KeyFrame::mnId + 1; a set is a
// hit only if its feature count, FeatureVector size and fingerprint are the key frame's (the identity rule of ORBmatcher's
// resident sets), so a key frame whose id Tracking::Reset has handed out again is put again.  Per call only the map-point
// flags, mvuRight, the shared nodes and one record per neighbour travel.  All neighbours of a call must share their
// mvScaleFactors / mvLevelSigma2 (in the reference they are copies of the one extractor's tables).
// Never throws; a failed device call is reported through hipdetail::Fail, the pair lists are left empty and 0 is returned
// (include/orbhip/hiperror.h).
#ifndef ORBHIP_TRIANGULATIONSEARCH_H
#define ORBHIP_TRIANGULATIONSEARCH_H

#include <mutex>
#include <utility>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include <opencv2/core/core.hpp>
#include "KeyFrame.h"
#else
#include "cvlite.h"
#include "slamlite.h"
#endif

struct orbhip_ctx;

namespace ORB_SLAM2
{

class TriangulationSearch
{
public:
    TriangulationSearch();                    // a device context of its own (a context is not re-entrant)
    ~TriangulationSearch();
    TriangulationSearch(const TriangulationSearch &) = delete;
    TriangulationSearch &operator=(const TriangulationSearch &) = delete;

    // Returns the number of matches over all neighbours.  vF12[k]: 3x3 CV_32F, LocalMapping::ComputeF12(pKF1, vpKF2[k]).
    int SearchForTriangulation(KeyFrame *pKF1, const std::vector<KeyFrame*> &vpKF2, const std::vector<cv::Mat> &vF12,
                               std::vector<std::vector<std::pair<size_t,size_t> > > &vvMatchedPairs,
                               bool bOnlyStereo, bool bCheckOrientation);

    // At most n key frames stay resident (clamped to 4 .. 96, the default); a call with more neighbours raises it to what it needs.
    void SetResidentSetLimit(int n);
    // Forgets every resident key frame (for Tracking::Reset; without it the fingerprint still catches a reused id).
    void DropResidentSets();

    // device of the objects constructed from now on (default 0)
    static void SetDevice(int device);

protected:
    orbhip_ctx *mpCtx;
    int mnSetLimit;                           // the limit the context runs with
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
