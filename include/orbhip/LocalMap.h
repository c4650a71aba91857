// LocalMap.h -- ORB_SLAM2::LocalMapSearch: the second half of Tracking::SearchLocalPoints (ref: src/Tracking.cc:2336-2364 --
// Frame::isInFrustum over mvpLocalMapPoints, then ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)) as one
// device call against map points that stay on the device (orbhip_map_*, orbhip_search_local_points; include/orbhip.h,
// DESIGN.md section 10).  No counterpart class in the reference: LocalMapping / LoopClosing tell it when a point changes (Put,
// UpdateFlags, Erase), Tracking calls SearchLocalPoints.  Never throws; a failed device call is
// reported through hipdetail::Fail and SearchLocalPoints returns 0 with nothing written (include/orbhip/hiperror.h).
#ifndef ORBHIP_LOCALMAP_H
#define ORBHIP_LOCALMAP_H

#include <mutex>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include "Frame.h"
#include "MapPoint.h"
#else
#include "slamlite.h"
#endif

struct orbhip_ctx;

namespace ORB_SLAM2
{

class LocalMapSearch
{
public:
    // a store for at most maxPoints map points, in a device context of its own (a context is not re-entrant)
    explicit LocalMapSearch(int maxPoints = 1 << 20);
    ~LocalMapSearch();
    LocalMapSearch(const LocalMapSearch &) = delete;
    LocalMapSearch &operator=(const LocalMapSearch &) = delete;

    // The point's position, normal, distance range, descriptor and flags as they are now (key MapPoint::mnId + 1): after
    // SetWorldPos, UpdateNormalAndDepth, ComputeDistinctiveDescriptors, and for every new point.  The vector form is one upload.
    void Put(MapPoint *pMP);
    void Put(const std::vector<MapPoint *> &vpMPs);
    // Observations() > 0 and isBad() alone: after AddObservation / EraseObservation / SetBadFlag
    void UpdateFlags(MapPoint *pMP);
    // after Replace and at the end of SetBadFlag
    void Erase(MapPoint *pMP);
    // from Tracking::Reset
    void Clear();

    // Leaves F.mvpMapPoints and, for every point of vpLocalMapPoints that is neither bad nor already seen in this frame
    // (mnLastFrameSeen == F.mnId), mbTrackInView / mTrackProjX / mTrackProjY / mTrackProjXR / mnTrackScaleLevel /
    // mTrackViewCos exactly as the reference's loop and SearchByProjection leave them.  IncreaseVisible() stays with the caller
    // (for the points with mbTrackInView).  *nToMatch = the number of points in view; returns the number of matches.
    int SearchLocalPoints(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, float th, float viewingCosLimit,
                          int *nToMatch);

    // device of the objects constructed from now on (default 0)
    static void SetDevice(int device);

protected:
    orbhip_ctx *mpCtx;
    std::mutex mMutex;
};

}  // namespace ORB_SLAM2

#endif
