// LocalMapCollect.cc -- Tracking::UpdateLocalMap through ORB_SLAM2::LocalMapSearch (include/orbhip/LocalMap.h): the key-frame
// table kept in step with KeyFrame::mvpMapPoints, the vote and the point union on the device, the covisibility step of
// UpdateLocalKeyFrames here on the caller's KeyFrame objects (ref: src/Tracking.cc:2367-2562).  A file of its own: programs
// that link LocalMap.cc alone need none of the orbhip_map_kf_* entry points.
#include <algorithm>
#include <set>

#include "LocalMapDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::call_with_room;
using localmapdetail::key_of;
using localmapdetail::room_for;

namespace
{
struct ById {
    bool operator()(KeyFrame *a, KeyFrame *b) const { return a->mnId < b->mnId; }
};
}  // namespace

void LocalMapSearch::InitKeyFrames(int maxKFs, int maxRow)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    mKeyFrameOf.clear();
    mbKeyFrames = orbhip_map_kf_init(mpCtx, maxKFs, maxRow) == ORBHIP_OK;
    if (!mbKeyFrames) hipdetail::Fail("LocalMapSearch::InitKeyFrames", orbhip_last_error(mpCtx));
}

bool LocalMapSearch::EnsureKeyFrames()
{
    if (!mpCtx) return false;
    if (mbKeyFrames) return true;
    mbKeyFrames = orbhip_map_kf_init(mpCtx, 4096, 2048) == ORBHIP_OK;
    if (!mbKeyFrames) hipdetail::Fail("LocalMapSearch (orbhip_map_kf_init)", orbhip_last_error(mpCtx));
    return mbKeyFrames;
}

void LocalMapSearch::PutKeyFrame(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    PutKeyFrameLocked(pKF);
}

bool LocalMapSearch::PutKeyFrameLocked(KeyFrame *pKF)
{
    if (!EnsureKeyFrames()) return false;
    const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();
    std::vector<uint64_t> row(vpMPs.size(), 0);
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *p = vpMPs[i];
        if (!p || !Known(p)) continue;
        if (p->GetIndexInKeyFrame(pKF) != (int)i) continue;   // the vector may hold a point twice; its observation names one index
        row[i] = key_of(p);
    }
    if (orbhip_map_kf_put(mpCtx, key_of(pKF), (int)row.size(), row.data()) != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch::PutKeyFrame", orbhip_last_error(mpCtx));
        return false;
    }
    mKeyFrameOf[key_of(pKF)] = pKF;
    return true;
}

void LocalMapSearch::SetMapPoint(KeyFrame *pKF, size_t idx, MapPoint *pMP)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EnsureKeyFrames()) return;
    const int32_t i = (int32_t)idx;
    const uint64_t key = pMP ? key_of(pMP) : 0;
    if (orbhip_map_kf_set(mpCtx, key_of(pKF), 1, &i, &key) != ORBHIP_OK) hipdetail::Fail("LocalMapSearch::SetMapPoint", orbhip_last_error(mpCtx));
}

void LocalMapSearch::EraseKeyFrame(KeyFrame *pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    EraseKeyFrameLocked(pKF, "LocalMapSearch::EraseKeyFrame");
}

bool LocalMapSearch::EraseKeyFrameLocked(KeyFrame *pKF, const char *who)
{
    if (!mpCtx || !mbKeyFrames) return false;
    mKeyFrameOf.erase(key_of(pKF));
    if (orbhip_map_kf_erase(mpCtx, key_of(pKF)) != ORBHIP_OK) hipdetail::Fail(who, orbhip_last_error(mpCtx));
    return true;
}

KeyFrame *LocalMapSearch::KeyFrameOf(uint64_t key) const
{
    const std::map<uint64_t, KeyFrame *>::const_iterator it = mKeyFrameOf.find(key);
    return it == mKeyFrameOf.end() ? static_cast<KeyFrame *>(NULL) : it->second;
}

bool LocalMapSearch::HasRow(KeyFrame *pKF) const { return KeyFrameOf(key_of(pKF)) == pKF; }

bool LocalMapSearch::CollectKeys(const std::vector<KeyFrame *> &vpKFs, std::vector<uint64_t> &kfKeys)
{
    // a key frame erased since the list was made (an empty vote keeps the last list) has no row: it adds nothing.  (Not HasRow: whose row is not asked)
    kfKeys.clear();
    for (size_t k = 0; k < vpKFs.size(); k++)
        if (mKeyFrameOf.count(key_of(vpKFs[k]))) kfKeys.push_back(key_of(vpKFs[k]));
    return true;
}

void LocalMapSearch::ClearKeyFrames()
{
    std::unique_lock<std::mutex> lock(mMutex);
    mKeyFrameOf.clear();
    mnLastVoted = mnLastLocal = 0;
    if (!mpCtx || !mbKeyFrames) return;
    if (orbhip_map_kf_clear(mpCtx) != ORBHIP_OK) hipdetail::Fail("LocalMapSearch::ClearKeyFrames", orbhip_last_error(mpCtx));
}

void LocalMapSearch::UpdateLocalMap(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints,
                                    KeyFrame *&pReferenceKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EnsureKeyFrames()) return;
    if (!VoteAndGraph(F, vpLocalKeyFrames, pReferenceKF)) return;

    // ---- UpdateLocalPoints (ref: :2377-2400) ----
    vpLocalMapPoints.clear();
    std::vector<uint64_t> kfKeys;
    CollectKeys(vpLocalKeyFrames, kfKeys);
    int nlocal = 0;
    std::vector<uint64_t> local;
    const int rc = call_with_room(room_for(mnLastLocal, mPointOf.size()), &nlocal, [&](int cap, size_t room) {
        local.resize(room);
        return orbhip_map_collect(mpCtx, (int)kfKeys.size(), kfKeys.data(), local.data(), cap, &nlocal);
    });
    if (rc != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch::UpdateLocalMap (orbhip_map_collect)", orbhip_last_error(mpCtx));
        return;
    }
    mnLastLocal = nlocal;
    vpLocalMapPoints.reserve(nlocal);
    for (int k = 0; k < nlocal; k++) {   // an unknown key is skipped here; TrackLocalPoints fails on one
        MapPoint *pMP = PointOf(local[k]);
        if (!pMP) continue;
        vpLocalMapPoints.push_back(pMP);
        pMP->mnTrackReferenceForFrame = F.mnId;
    }
}

void LocalMapSearch::UpdateLocalKeyFrames(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, KeyFrame *&pReferenceKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EnsureKeyFrames()) return;
    VoteAndGraph(F, vpLocalKeyFrames, pReferenceKF);
}

bool LocalMapSearch::VoteAndGraph(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, KeyFrame *&pReferenceKF)
{
    // ---- UpdateLocalKeyFrames: the vote (ref: :2411-2429) ----
    std::vector<uint64_t> frameKeys(F.N > 0 ? F.N : 0, 0);
    for (int i = 0; i < F.N; i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad())
            F.mvpMapPoints[i] = static_cast<MapPoint *>(NULL);
        else
            frameKeys[i] = key_of(pMP);
    }
    int nvoted = 0;
    std::vector<uint64_t> votedKeys;
    std::vector<int32_t> votes;
    const int rc = call_with_room(room_for(mnLastVoted, mKeyFrameOf.size()), &nvoted, [&](int cap, size_t room) {
        votedKeys.resize(room), votes.resize(room);
        return orbhip_map_vote(mpCtx, (int)frameKeys.size(), frameKeys.data(), votedKeys.data(), votes.data(), cap, &nvoted);
    });
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::UpdateLocalMap (orbhip_map_vote)", orbhip_last_error(mpCtx)), false;
    mnLastVoted = nvoted;

    if (nvoted > 0) {   // (keyframeCounter.empty(): the reference returns and keeps the lists it has)
        int max = 0;
        KeyFrame *pKFmax = static_cast<KeyFrame *>(NULL);
        vpLocalKeyFrames.clear();
        vpLocalKeyFrames.reserve(3 * nvoted);
        // ---- key frames that share points with the frame, in ascending mnId order (ref: :2445-2461) ----
        for (int k = 0; k < nvoted; k++) {
            KeyFrame *pKF = KeyFrameOf(votedKeys[k]);
            if (!pKF || pKF->isBad()) continue;
            if (votes[k] > max) {
                max = votes[k];
                pKFmax = pKF;
            }
            vpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = F.mnId;
        }
        // ---- one neighbour, one child, the parent of each of them (ref: :2467-2527; the reference's iterators were taken
        // before it appends, so only the key frames above are visited) ----
        const size_t nShared = vpLocalKeyFrames.size();
        for (size_t k = 0; k < nShared; k++) {
            if (vpLocalKeyFrames.size() > 80) break;
            KeyFrame *pKF = vpLocalKeyFrames[k];
            const std::vector<KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (std::vector<KeyFrame *>::const_iterator itN = vNeighs.begin(); itN != vNeighs.end(); itN++) {
                KeyFrame *pNeighKF = *itN;
                if (!pNeighKF->isBad() && pNeighKF->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            }
            const std::set<KeyFrame *> spChilds = pKF->GetChilds();
            std::vector<KeyFrame *> vChilds(spChilds.begin(), spChilds.end());
            std::sort(vChilds.begin(), vChilds.end(), ById());   // (the reference walks the set by heap address)
            for (std::vector<KeyFrame *>::const_iterator sit = vChilds.begin(); sit != vChilds.end(); sit++) {
                KeyFrame *pChildKF = *sit;
                if (!pChildKF->isBad() && pChildKF->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(pChildKF);
                    pChildKF->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            }
            KeyFrame *pParent = pKF->GetParent();
            if (pParent && pParent->mnTrackReferenceForFrame != F.mnId) {
                vpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = F.mnId;
                break;   // ref: :2524 -- the monocular branch leaves the loop over the key frames here
            }
        }
        if (pKFmax) pReferenceKF = pKFmax;
    }

    return true;
}

int LocalMapSearch::TrackLocalPoints(Frame &F, const std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints,
                                     float th, float viewingCosLimit, int *nToMatch)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (nToMatch) *nToMatch = 0;
    vpLocalMapPoints.clear();
    if (!EnsureKeyFrames()) return 0;
    if (!localmapdetail::has_pyramid(F))
        return hipdetail::Fail("LocalMapSearch::TrackLocalPoints", "the frame has no scale pyramid (mnScaleLevels, mvScaleFactors)"), 0;
    const int n = F.N;
    uint64_t frameKey = 0;
    if (!localmapdetail::put_frame(mpCtx, F, &frameKey))
        return hipdetail::Fail("LocalMapSearch::TrackLocalPoints (orbhip_set_put)", orbhip_last_error(mpCtx)), 0;
    orbhip_local_camera cam;
    localmapdetail::fill_camera(F, th, viewingCosLimit, &cam);
    std::vector<uint8_t> occupied;
    localmapdetail::fill_occupied(F, occupied);
    std::vector<uint64_t> kfKeys, seen;
    CollectKeys(vpLocalKeyFrames, kfKeys);
    for (int i = 0; i < n; i++)   // the frame's own matches (ref: :2318-2334 stamps them with mnLastFrameSeen)
        if (F.mvpMapPoints[i] && F.mvpMapPoints[i]->mnLastFrameSeen == F.mnId) seen.push_back(key_of(F.mvpMapPoints[i]));
    const std::set<uint64_t> seenSet(seen.begin(), seen.end());
    int nlocal = 0, ntm = 0, found = 0;
    std::vector<uint64_t> local;
    std::vector<orbhip_local_point> pts;
    std::vector<int32_t> match(n > 0 ? n : 1);
    // the result block that comes back is sized by cap, not by the list: keep cap near the list
    const int rc = call_with_room(room_for(mnLastLocal, mPointOf.size()), &nlocal, [&](int cap, size_t room) {
        local.resize(room), pts.resize(room);
        return orbhip_track_local_points(mpCtx, frameKey, (n > 0 && (int)F.mvuRight.size() == n) ? F.mvuRight.data() : NULL,
                                         occupied.data(), &cam, (int)kfKeys.size(), kfKeys.data(), (int)seen.size(), seen.data(), 0.8f,
                                         local.data(), cap, &nlocal, pts.data(), &ntm, match.data(), &found);
    });
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::TrackLocalPoints", orbhip_last_error(mpCtx)), 0;
    mnLastLocal = nlocal;
    std::vector<uint8_t> skip(nlocal);
    vpLocalMapPoints.reserve(nlocal);
    for (int k = 0; k < nlocal; k++) {   // an unknown key fails here; UpdateLocalMap skips one
        MapPoint *pMP = PointOf(local[k]);
        if (!pMP) return hipdetail::Fail("LocalMapSearch::TrackLocalPoints", "a local point was never Put"), 0;
        vpLocalMapPoints.push_back(pMP);
        pMP->mnTrackReferenceForFrame = F.mnId;
        skip[k] = seenSet.count(local[k]) ? 1 : 0;   // what the device skipped: the same list, not the stamp
    }
    pts.resize(nlocal);
    localmapdetail::write_back(F, vpLocalMapPoints, skip, pts, match);
    if (nToMatch) *nToMatch = ntm;
    return found;
}

}  // namespace ORB_SLAM2
