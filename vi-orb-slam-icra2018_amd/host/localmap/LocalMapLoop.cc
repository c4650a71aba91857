// LocalMapLoop.cc -- LoopClosing's two projection searches through ORB_SLAM2::LocalMapSearch (include/orbhip/LocalMap.h; ref:
// src/LoopClosing.cc:404-427, :647-673, src/ORBmatcher.cc:290-403, :977-1100): SearchLoopPoints and SearchAndFuse as one device
// call each (per 64 targets) against the resident store, key-frame table and feature sets (orbhip_search_loop_points,
// orbhip_fuse_sim3), the map edits here on the caller's objects in the reference's order, and the resident
// state brought up to date once per device call, the table with one orbhip_map_kf_set_batch.  A file of its own: programs that
// link the other LocalMap*.cc files alone need none of the three entry points.
#include <algorithm>

#include "LocalMapDetail.h"
#include "../MatcherDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::call_with_room;
using localmapdetail::fill_target;
using localmapdetail::has_pyramid;
using localmapdetail::key_of;
using localmapdetail::room_for;

namespace
{
const int LOOP_CHUNK = 64;   // targets per device call, as FuseInTargets
const int TH_LOW = 50;       // ORBmatcher::TH_LOW

// the target with Rcw, tcw, Ow of the similarity (ref: src/ORBmatcher.cc:299-303, :986-990)
void fill_sim3_target(KeyFrame *pKF, uint64_t setKey, const cv::Mat &Scw, float th, orbhip_fuse_target *out)
{
    fill_target(pKF, setKey, th, out);
    cv::Mat Rcw;
    hipdetail::decompose_sim3(Scw, Rcw, out->cam.tcw, out->cam.Ow);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out->cam.Rcw[3 * r + c] = Rcw.at<float>(r, c);
}
}  // namespace

bool LocalMapSearch::FlushLoop(FuseEdits &edits)
{
    FuseRows rows;
    bool ok = TakeFuseEdits(edits, rows);
    std::vector<uint64_t> kf, pt;
    std::vector<int32_t> idx;
    for (FuseRows::const_iterator it = rows.begin(); it != rows.end(); ++it) {
        kf.insert(kf.end(), it->second.first.size(), it->first);
        idx.insert(idx.end(), it->second.first.begin(), it->second.first.end());
        pt.insert(pt.end(), it->second.second.begin(), it->second.second.end());
    }
    if (!kf.empty() && orbhip_map_kf_set_batch(mpCtx, (int)kf.size(), kf.data(), idx.data(), pt.data()) != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch::SearchAndFuse (orbhip_map_kf_set_batch)", orbhip_last_error(mpCtx));
        ok = false;
    }
    return ok;
}

int LocalMapSearch::SearchLoopPoints(KeyFrame *pCurrentKF, const cv::Mat &Scw, const std::vector<KeyFrame *> &vpLoopConnectedKFs,
                                     std::vector<MapPoint *> &vpLoopMapPoints, std::vector<MapPoint *> &vpCurrentMatchedPoints, int th)
{
    std::unique_lock<std::mutex> lock(mMutex);
    vpLoopMapPoints.clear();                                                        // ref: src/LoopClosing.cc:407
    if (!EnsureKeyFrames()) return 0;
    if (!has_pyramid(pCurrentKF))
        return hipdetail::Fail("LocalMapSearch::SearchLoopPoints", "the key frame has no scale pyramid (mnScaleLevels, mvScaleFactors, mvInvLevelSigma2)"), 0;
    const int n = (int)pCurrentKF->mvKeysUn.size();
    if ((int)vpCurrentMatchedPoints.size() != n)
        return hipdetail::Fail("LocalMapSearch::SearchLoopPoints", "vpCurrentMatchedPoints is not as long as the key frame's features"), 0;
    for (size_t k = 0; k < vpLoopConnectedKFs.size(); k++)
        if (!EnsureRow(vpLoopConnectedKFs[k])) return 0;
    std::vector<uint64_t> kfKeys;
    CollectKeys(vpLoopConnectedKFs, kfKeys);
    if (n == 0 || kfKeys.empty()) return 0;
    uint64_t setKey = 0;
    if (!EnsureFuseSet(pCurrentKF, &setKey)) return hipdetail::Fail("LocalMapSearch::SearchLoopPoints (key frame set)", orbhip_last_error(mpCtx)), 0;
    orbhip_fuse_target target;
    fill_sim3_target(pCurrentKF, setKey, Scw, (float)th, &target);
    std::vector<uint64_t> matched(n, 0);                                            // vpMatched as keys (ref: src/ORBmatcher.cc:306-307, :375)
    for (int i = 0; i < n; i++)
        if (vpCurrentMatchedPoints[i]) matched[i] = key_of(vpCurrentMatchedPoints[i]);
    int npoints = 0, nActive = 0, nmatches = 0;
    std::vector<uint64_t> keys;
    std::vector<int32_t> match(n);
    const int rc = call_with_room(room_for(mnLastLoopPoints, mPointOf.size()), &npoints, [&](int cap, size_t room) {
        keys.resize(room);
        return orbhip_search_loop_points(mpCtx, &target, (int)kfKeys.size(), kfKeys.data(), matched.data(), TH_LOW, keys.data(), cap, &npoints,
                                         NULL, &nActive, match.data(), &nmatches);
    });
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::SearchLoopPoints", orbhip_last_error(mpCtx)), 0;
    mnLastLoopPoints = npoints;
    PointsOf(keys.data(), npoints, vpLoopMapPoints);                                // ref: src/LoopClosing.cc:408-424, element for element
    for (int i = 0; i < n; i++)
        if (match[i] >= 0 && match[i] < npoints) vpCurrentMatchedPoints[i] = vpLoopMapPoints[match[i]];   // ref: src/ORBmatcher.cc:396
    return nmatches;
}

void LocalMapSearch::SearchAndFuse(const std::vector<std::pair<KeyFrame *, cv::Mat> > &vCorrectedPoses,
                                   const std::vector<MapPoint *> &vpLoopMapPoints, float th)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const int K = (int)vCorrectedPoses.size(), n = (int)vpLoopMapPoints.size();
    if (K == 0 || n == 0 || !EnsureKeyFrames()) return;
    LoopPhases &ph = Phases();
    localmapdetail::Stopwatch watch;
    for (int k = 0; k < K; k++) {
        KeyFrame *pKF = vCorrectedPoses[k].first;
        if (!has_pyramid(pKF))
            return (void)hipdetail::Fail("LocalMapSearch::SearchAndFuse", "a key frame has no scale pyramid (mnScaleLevels, mvScaleFactors, mvInvLevelSigma2)");
        if (!EnsureRow(pKF)) return;
    }
    std::vector<uint64_t> pointKeys(n, 0);           // a point that was never Put, or that the list names a second time, takes no part
    {
        std::set<MapPoint *> seen;
        for (int i = 0; i < n; i++)
            if (vpLoopMapPoints[i] && Known(vpLoopMapPoints[i]) && seen.insert(vpLoopMapPoints[i]).second)
                pointKeys[i] = key_of(vpLoopMapPoints[i]);
    }
    FuseEdits edits;
    std::vector<orbhip_fuse_target> targets;
    std::vector<uint64_t> rowKeys;
    std::vector<orbhip_proj_query> queries;
    std::vector<int32_t> bestIdx, bestDist, nActive;
    std::vector<int> redo;
    localmapdetail::ResearchBuffers again;
    std::vector<MapPoint *> vpReplacePoints;
    for (int start = 0; start < K; start += LOOP_CHUNK) {
        const int cnt = std::min(LOOP_CHUNK, K - start);
        targets.resize(cnt), rowKeys.resize(cnt);
        for (int j = 0; j < cnt; j++) {
            KeyFrame *pKF = vCorrectedPoses[start + j].first;
            uint64_t setKey = 0;
            if (!EnsureFuseSet(pKF, &setKey)) return (void)hipdetail::Fail("LocalMapSearch::SearchAndFuse (key frame set)", orbhip_last_error(mpCtx));
            fill_sim3_target(pKF, setKey, vCorrectedPoses[start + j].second, th, &targets[j]);
            rowKeys[j] = key_of(pKF);
        }
        const size_t total = (size_t)cnt * n;
        queries.resize(total), bestIdx.resize(total), bestDist.resize(total), nActive.resize(cnt);
        watch.lap(&ph.prepare);
        if (orbhip_fuse_sim3(mpCtx, targets.data(), rowKeys.data(), cnt, pointKeys.data(), n, queries.data(), bestIdx.data(), bestDist.data(),
                             nActive.data()) != ORBHIP_OK)
            return (void)hipdetail::Fail("LocalMapSearch::SearchAndFuse", orbhip_last_error(mpCtx));
        watch.lap(&ph.device);
        for (int j = 0; j < cnt; j++) {
            KeyFrame *pKF = vCorrectedPoses[start + j].first;
            const orbhip_proj_query *Q = &queries[(size_t)j * n];
            int32_t *bi = &bestIdx[(size_t)j * n], *bd = &bestDist[(size_t)j * n];
            const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();          // ref: src/ORBmatcher.cc:993, as it is NOW
            const int nFeat = (int)pKF->GetMapPointMatches().size();
            // loop points whose descriptor changed since the call (they survived a Replace in an earlier target): their windows
            // are what they were, their best feature may not be.  (FuseInTargets asks less of a point, and searches with uRight and sigmas)
            redo.clear();
            for (int i = 0; i < n && !edits.survivors.empty() && ResearchChangedSurvivors(); i++) {
                MapPoint *pMP = vpLoopMapPoints[i];
                if (!(Q[i].flags & ORBHIP_Q_ACTIVE) || !pointKeys[i] || pMP->isBad() || spAlreadyFound.count(pMP)) continue;
                if (edits.ChangedSince(pMP)) redo.push_back(i);
            }
            if (!redo.empty() && !localmapdetail::research_survivors(mpCtx, redo, Q, vpLoopMapPoints, targets[j].set_key, NULL, NULL, 0, bi, bd, again))
                return (void)hipdetail::Fail("LocalMapSearch::SearchAndFuse (orbhip_window_best_set)", orbhip_last_error(mpCtx));
            watch.lap(&ph.research);
            // ref: src/ORBmatcher.cc:1081-1096 over the results, in list order
            vpReplacePoints.assign(n, static_cast<MapPoint *>(NULL));                 // ref: src/LoopClosing.cc:658
            for (int i = 0; i < n; i++) {
                MapPoint *pMP = vpLoopMapPoints[i];
                if (!pointKeys[i] || !(Q[i].flags & ORBHIP_Q_ACTIVE)) continue;
                if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;              // ref: :1005
                if (bi[i] < 0 || bi[i] >= nFeat || bd[i] > TH_LOW) continue;
                const size_t feat = (size_t)bi[i];
                MapPoint *pMPinKF = pKF->GetMapPoint(feat);
                if (pMPinKF) {
                    if (!pMPinKF->isBad()) vpReplacePoints[i] = pMPinKF;
                } else {
                    pMP->AddObservation(pKF, feat);
                    pKF->AddMapPoint(pMP, feat);
                    edits.entries.insert(std::make_pair(pKF, feat));
                    edits.flags.insert(pMP);
                }
            }
            // ref: src/LoopClosing.cc:663-671
            for (int i = 0; i < n; i++) {
                MapPoint *pRep = vpReplacePoints[i], *pMP = vpLoopMapPoints[i];
                if (pRep) edits.Replace(pRep, pMP);
            }
            watch.lap(&ph.apply);
        }
        const bool flushed = FlushLoop(edits);           // once per device call
        watch.lap(&ph.resident);
        if (!flushed) return;
        edits.survivors.clear();                         // the store has their descriptors now
    }
}

}  // namespace ORB_SLAM2
