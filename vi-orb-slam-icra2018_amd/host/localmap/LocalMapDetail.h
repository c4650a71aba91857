// LocalMapDetail.h -- what the LocalMap*.cc files of this directory share and need no member of the class for (the shared members
// are in the protected part of LocalMap.h; DESIGN.md section 27 lists both): keys and flags of a MapPoint, the room a call offers and
// the call made again, the frame as a resident set, the camera block of a search and the write-back of its results (ref:
// src/Tracking.cc:2336-2364, src/Frame.cc:613-669, src/ORBmatcher.cc:45-129), the Fuse target, what the two refreshes share.
#ifndef ORBHIP_LOCALMAP_DETAIL_H
#define ORBHIP_LOCALMAP_DETAIL_H

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "LocalMap.h"
#include "orbhip.h"

namespace ORB_SLAM2
{
namespace localmapdetail
{
inline uint64_t key_of(MapPoint *pMP) { return (uint64_t)pMP->mnId + 1; }
inline uint64_t key_of(KeyFrame *pKF) { return (uint64_t)pKF->mnId + 1; }
// a key frame's feature set, apart from the frames' (Frame::mnId + 1)
inline uint64_t set_key_of(KeyFrame *pKF) { return (1ull << 62) | key_of(pKF); }
inline uint8_t flags_of(MapPoint *pMP)
{
    return (uint8_t)((pMP->Observations() > 0 ? ORBHIP_MP_OBSERVED : 0) | (pMP->isBad() ? ORBHIP_MP_BAD : 0));
}

// room for a list that is usually about as long as the last one: a quarter more and `slack`, never more than `most` (the list is
// a function of the map, never of the room)
inline int room_for(size_t last, size_t most, size_t slack = 256) { return (int)std::min(most, last + last / 4 + slack); }

// call(cap, room) sizes its buffers for `room` elements (cap, but one for cap 0) and makes the call, which reports the list's size in
// *reported.  While it answers ORBHIP_E_CAPACITY and reports more than cap, it is made again with exactly that.  Returns the last code.
template <class Call> int call_with_room(int cap, const int *reported, Call call)
{
    int rc;
    while ((rc = call(cap, (size_t)(cap > 0 ? cap : 1))) == ORBHIP_E_CAPACITY && *reported > cap) cap = *reported;
    return rc;
}

// adds the time since the last lap (or its construction) to a sum of microseconds
struct Stopwatch {
    std::chrono::steady_clock::time_point t0;
    Stopwatch() : t0(std::chrono::steady_clock::now()) {}
    void lap(double *sum)
    {
        const std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
        *sum += std::chrono::duration<double, std::micro>(t1 - t0).count();
        t0 = t1;
    }
};

inline bool has_pyramid(const Frame &F) { return F.mnScaleLevels >= 1 && F.mnScaleLevels <= 16 && (int)F.mvScaleFactors.size() >= F.mnScaleLevels; }

// the frame as a resident set with a grid, under Frame::mnId + 1 (0 for a frame without features): uploaded the first time the
// frame is searched
inline bool put_frame(orbhip_ctx *ctx, Frame &F, uint64_t *frameKey)
{
    const int n = F.N;
    *frameKey = n > 0 ? (uint64_t)F.mnId + 1 : 0;
    if (n > 0 && !orbhip_set_has(ctx, *frameKey, n)) {
        std::vector<uint8_t> d((size_t)n * 32);
        for (int i = 0; i < n; i++) memcpy(&d[(size_t)i * 32], F.mDescriptors.ptr(i), 32);
        if (orbhip_set_put(ctx, *frameKey, reinterpret_cast<const orbhip_keypoint *>(F.mvKeysUn.data()), d.data(), n, NULL, NULL, NULL,
                           0, Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv) != ORBHIP_OK)
            return false;
    }
    return true;
}

inline void fill_camera(Frame &F, float th, float viewingCosLimit, orbhip_local_camera *out)
{
    orbhip_local_camera &cam = *out;
    memset(&cam, 0, sizeof cam);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rcw[3 * r + c] = F.mTcw.at<float>(r, c);    // mRcw, mtcw (ref: Frame::UpdatePoseMatrices)
        cam.tcw[r] = F.mTcw.at<float>(r, 3);
    }
    // mOw = -mRcw.t()*mtcw: one gemm with alpha = -1, summed in double, one rounding.  Not hipdetail::affine3(.., true, -1.0): that
    // rounds alpha * s + 0.0, which is +0.0 where this is -0.0, and the sign reaches the device (tests/test_localmap_zero_dot.py)
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)cam.Rcw[3 * k + r] * (double)cam.tcw[k];
        cam.Ow[r] = (float)(-1.0 * s);
    }
    cam.fx = Frame::fx, cam.fy = Frame::fy, cam.cx = Frame::cx, cam.cy = Frame::cy, cam.mbf = F.mbf;
    cam.min_x = Frame::mnMinX, cam.max_x = Frame::mnMaxX, cam.min_y = Frame::mnMinY, cam.max_y = Frame::mnMaxY;
    for (int l = 0; l < F.mnScaleLevels; l++) cam.scale_factors[l] = F.mvScaleFactors[l];
    cam.log_scale_factor = F.mfLogScaleFactor;
    cam.nlevels = F.mnScaleLevels;
    cam.viewing_cos_limit = viewingCosLimit;
    cam.th = th;
}

// occupied[i] = the feature holds a point with observations (ref: src/ORBmatcher.cc:87-89)
inline void fill_occupied(Frame &F, std::vector<uint8_t> &occupied)
{
    occupied.assign(F.N > 0 ? F.N : 1, 0);
    for (int i = 0; i < F.N; i++)
        if (F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0) occupied[i] = 1;
}

inline void write_back(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, const std::vector<uint8_t> &skip,
                       const std::vector<orbhip_local_point> &pts, const std::vector<int32_t> &match)
{
    const int n = F.N, nq = (int)vpLocalMapPoints.size();
    for (int k = 0; k < nq; k++) {
        MapPoint *p = vpLocalMapPoints[k];
        if (skip[k] || p->isBad()) continue;                   // ref: :2342-2345 -- the loop does not touch these
        p->mbTrackInView = pts[k].in_view != 0;                // ref: src/Frame.cc:615
        if (!pts[k].in_view) continue;
        p->mTrackProjX = pts[k].u;                             // ref: :661-666
        p->mTrackProjXR = pts[k].proj_xr;
        p->mTrackProjY = pts[k].v;
        p->mnTrackScaleLevel = pts[k].level;
        p->mTrackViewCos = pts[k].view_cos;
    }
    for (int i = 0; i < n; i++)
        if (match[i] >= 0 && match[i] < nq) F.mvpMapPoints[i] = vpLocalMapPoints[match[i]];   // ref: src/ORBmatcher.cc:123
}
// ---- the target key frames of the Fuse calls (LocalMapFuse.cc, LocalMapLoop.cc) ----
inline bool has_pyramid(KeyFrame *pKF)
{
    return pKF->mnScaleLevels >= 1 && pKF->mnScaleLevels <= 16 && (int)pKF->mvScaleFactors.size() >= pKF->mnScaleLevels &&
           (int)pKF->mvInvLevelSigma2.size() >= pKF->mnScaleLevels;
}

// the target key frame as Fuse reads it (ref: src/ORBmatcher.cc:827-838)
inline void fill_target(KeyFrame *pKF, uint64_t setKey, float th, orbhip_fuse_target *out)
{
    memset(out, 0, sizeof *out);
    out->set_key = setKey;
    orbhip_local_camera &cam = out->cam;
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) cam.Rcw[3 * r + c] = R.at<float>(r, c);
        cam.tcw[r] = t.at<float>(r, 0);
        cam.Ow[r] = O.at<float>(r, 0);
    }
    cam.fx = pKF->fx, cam.fy = pKF->fy, cam.cx = pKF->cx, cam.cy = pKF->cy, cam.mbf = pKF->mbf;
    cam.min_x = pKF->mnMinX, cam.max_x = pKF->mnMaxX, cam.min_y = pKF->mnMinY, cam.max_y = pKF->mnMaxY;
    for (int l = 0; l < pKF->mnScaleLevels; l++) {
        cam.scale_factors[l] = pKF->mvScaleFactors[l];
        out->inv_level_sigma2[l] = pKF->mvInvLevelSigma2[l];
    }
    cam.log_scale_factor = pKF->mfLogScaleFactor;
    cam.nlevels = pKF->mnScaleLevels;
    cam.th = th;
}

// The second search of one target (LocalMapFuse.cc; for FuseInTargets and SearchAndFuse): the queries Q[redo[k]] with the descriptors
// vpMPs[redo[k]] have now, in the target's set; results go to bestIdx / bestDist at redo[k].  false: the call failed.  b: kept by the caller.
struct ResearchBuffers { std::vector<orbhip_proj_query> q; std::vector<uint8_t> qdesc; std::vector<int32_t> idx, dist; };
bool research_survivors(orbhip_ctx *ctx, const std::vector<int> &redo, const orbhip_proj_query *Q, const std::vector<MapPoint *> &vpMPs,
                        uint64_t setKey, const float *uRight, const float *invLevelSigma2, int nlevels, int32_t *bestIdx, int32_t *bestDist,
                        ResearchBuffers &b);

// ---- RefreshPoints and CorrectLoopPoints (LocalMapRefresh.cc, LocalMapCorrect.cc) ----
// a point's observations in ascending KeyFrame::mnId (the reference walks the map by heap address; docs/parity.md)
typedef std::vector<std::pair<KeyFrame *, size_t> > ObservationList;
inline ObservationList observations_by_mnid(MapPoint *pMP)
{
    struct ByMnId {
        bool operator()(const std::pair<KeyFrame *, size_t> &a, const std::pair<KeyFrame *, size_t> &b) const { return a.first->mnId < b.first->mnId; }
    };
    const std::map<KeyFrame *, size_t> obs = pMP->GetObservations();
    ObservationList l(obs.begin(), obs.end());
    std::sort(l.begin(), l.end(), ByMnId());
    return l;
}

// the scale pyramid of the session, from one of its key frames; everything else zero
inline void fill_refresh_params(KeyFrame *pyramid, orbhip_refresh_params *prm)
{
    memset(prm, 0, sizeof *prm);
    for (int l = 0; l < pyramid->mnScaleLevels; l++) prm->scale_factors[l] = pyramid->mvScaleFactors[l];
    prm->nlevels = pyramid->mnScaleLevels;
}
}  // namespace localmapdetail
}  // namespace ORB_SLAM2

#endif
