// LocalMapProjTrack.cc -- Tracking's two other projection searches through ORB_SLAM2::LocalMapSearch (include/orbhip/LocalMap.h):
// SearchLastFrame (TrackWithMotionModel, ref: src/ORBmatcher.cc:1341-1498) and SearchKeyFramePoints (Relocalization, ref:
// :1500-1627) as one device call each against the resident store, key-frame table and feature sets (orbhip_search_last_frame,
// orbhip_search_keyframe_points).  A file of its own: programs that link LocalMap.cc and
// LocalMapCollect.cc alone need neither entry point.
#include <algorithm>

#include "LocalMapDetail.h"
#include "../MatcherDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::has_pyramid;
using localmapdetail::key_of;

namespace
{
// match[] of the window search -> Cur.mvpMapPoints the way the reference's loops write it (ref: :1452, :1489, :1579, :1617)
void write_matches(Frame &Cur, const std::vector<int32_t> &match, const std::vector<MapPoint *> &source)
{
    for (int i = 0; i < Cur.N; i++) {
        if (match[i] >= 0 && match[i] < (int)source.size())
            Cur.mvpMapPoints[i] = source[match[i]];
        else if (match[i] == -2)
            Cur.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
    }
}
}  // namespace

int LocalMapSearch::SearchLastFrame(Frame &Cur, const Frame &Last, float th, bool bMono, bool checkOri)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return 0;
    const int n = Cur.N, nq = Last.N;
    if (n == 0 || nq == 0) return 0;
    if (!has_pyramid(Cur)) return hipdetail::Fail("LocalMapSearch::SearchLastFrame", "the frame has no scale pyramid (mnScaleLevels, mvScaleFactors)"), 0;

    // the current camera's centre in the last camera's frame: forward or backward by more than the baseline (ref: :1351-1365)
    const cv::Mat Rcw = Cur.mTcw.rowRange(0, 3).colRange(0, 3), Rlw = Last.mTcw.rowRange(0, 3).colRange(0, 3);
    float tcw[3], tlw[3], twc[3], tlc[3];
    for (int r = 0; r < 3; r++) tcw[r] = Cur.mTcw.at<float>(r, 3), tlw[r] = Last.mTcw.at<float>(r, 3);
    hipdetail::affine3(Rcw, tcw, NULL, twc, true, -1.0);
    hipdetail::affine3(Rlw, twc, tlw, tlc);
    int motion = 0;
    if (!bMono && tlc[2] > Cur.mb) motion = 1;
    else if (!bMono && -tlc[2] > Cur.mb) motion = 2;

    uint64_t curKey = 0, lastKey = 0;
    if (!localmapdetail::put_frame(mpCtx, Cur, &curKey) || !localmapdetail::put_frame(mpCtx, const_cast<Frame &>(Last), &lastKey))
        return hipdetail::Fail("LocalMapSearch::SearchLastFrame (orbhip_set_put)", orbhip_last_error(mpCtx)), 0;

    std::vector<uint64_t> keys(nq, 0);
    std::vector<MapPoint *> fresh;      // points the store does not know: Tracking's temporal stereo points
    for (int i = 0; i < nq; i++) {
        MapPoint *p = Last.mvpMapPoints[i];
        if (!p || Last.mvbOutlier[i]) continue;                   // ref: :1370-1372
        keys[i] = key_of(p);
        if (!Known(p) && std::find(fresh.begin(), fresh.end(), p) == fresh.end()) fresh.push_back(p);
    }
    if (!PutLocked(fresh)) return 0;

    orbhip_local_camera cam;
    localmapdetail::fill_camera(Cur, th, 0.f, &cam);
    std::vector<uint8_t> occupied;
    localmapdetail::fill_occupied(Cur, occupied);                 // ref: :1413-1415
    std::vector<int32_t> match(n);
    int found = 0;
    const int rc = orbhip_search_last_frame(mpCtx, curKey, lastKey, keys.data(), nq, &cam, motion,
                                            (int)Cur.mvuRight.size() == n ? Cur.mvuRight.data() : NULL, occupied.data(), checkOri ? 1 : 0,
                                            100 /* ORBmatcher::TH_HIGH */, NULL, NULL, match.data(), &found);
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::SearchLastFrame", orbhip_last_error(mpCtx)), 0;
    write_matches(Cur, match, Last.mvpMapPoints);
    return found;
}

int LocalMapSearch::SearchKeyFramePoints(Frame &Cur, KeyFrame *pKF, const std::set<MapPoint *> &sAlreadyFound, float th, int ORBdist,
                                         bool checkOri)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EnsureKeyFrames()) return 0;
    const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();
    const int n = Cur.N, nq = (int)vpMPs.size();
    if (n == 0 || nq == 0) return 0;
    if (!has_pyramid(Cur)) return hipdetail::Fail("LocalMapSearch::SearchKeyFramePoints", "the frame has no scale pyramid (mnScaleLevels, mvScaleFactors)"), 0;
    if (!EnsureRow(pKF)) return 0;

    uint64_t curKey = 0;
    if (!localmapdetail::put_frame(mpCtx, Cur, &curKey))
        return hipdetail::Fail("LocalMapSearch::SearchKeyFramePoints (orbhip_set_put)", orbhip_last_error(mpCtx)), 0;
    const uint64_t kfSetKey = localmapdetail::set_key_of(pKF);   // (not EnsureFuseSet: that raises the set limit on first use)
    if (!hipdetail::ensure_set(mpCtx, kfSetKey, *pKF, pKF->mvKeysUn, pKF->mnMinX, pKF->mnMinY, pKF->mfGridElementWidthInv,
                               pKF->mfGridElementHeightInv, NULL))
        return hipdetail::Fail("LocalMapSearch::SearchKeyFramePoints (key frame set)", orbhip_last_error(mpCtx)), 0;

    std::vector<uint64_t> foundKeys;
    foundKeys.reserve(sAlreadyFound.size());
    for (std::set<MapPoint *>::const_iterator it = sAlreadyFound.begin(); it != sAlreadyFound.end(); ++it)
        if (*it) foundKeys.push_back(key_of(*it));                // ref: :1522

    orbhip_local_camera cam;
    localmapdetail::fill_camera(Cur, th, 0.f, &cam);
    std::vector<uint8_t> occupied(n, 0);
    for (int i = 0; i < n; i++)
        if (Cur.mvpMapPoints[i]) occupied[i] = 1;                 // ref: :1565-1566 (any point closes the feature)
    std::vector<int32_t> match(n);
    int found = 0;
    const int rc = orbhip_search_keyframe_points(mpCtx, curKey, kfSetKey, key_of(pKF), foundKeys.data(), (int)foundKeys.size(), &cam,
                                                 occupied.data(), checkOri ? 1 : 0, ORBdist, NULL, NULL, match.data(), &found);
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::SearchKeyFramePoints", orbhip_last_error(mpCtx)), 0;
    write_matches(Cur, match, vpMPs);
    return found;
}

}  // namespace ORB_SLAM2
