// LocalMapFuse.cc -- the two Fuse loops of LocalMapping::SearchInNeighbors through ORB_SLAM2::LocalMapSearch
// (include/orbhip/LocalMap.h; ref: src/LocalMapping.cc:2549-2581, src/ORBmatcher.cc:825-975): FuseInTargets and FuseCandidates as
// one device call each against the resident store, key-frame table and feature sets (orbhip_fuse_row, orbhip_fuse_collect;
// DESIGN.md section 17), the map edits here on the caller's objects in the reference's order, and the resident state brought up
// to date with every edit.  A file of its own: programs that link the other LocalMap*.cc files alone need neither entry point.
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
using localmapdetail::set_key_of;

namespace
{
const uint64_t SNAPSHOT_ROW = 1ull << 61;   // the source list as it was when FuseInTargets began (calls of more than FUSE_CHUNK targets)
const int FUSE_CHUNK = 64;                  // targets per device call: their sets stay resident beside the frames being tracked
const int FUSE_SETS = 96;                   // the set limit from the first FuseInTargets on
const int TH_LOW = 50;                      // ORBmatcher::TH_LOW

bool is_stereo(KeyFrame *pKF) { return !pKF->mvKeysUn.empty() && pKF->mvuRight.size() == pKF->mvKeysUn.size(); }
}  // namespace

bool LocalMapSearch::EnsureFuseSet(KeyFrame *pKF, uint64_t *setKey)
{
    if (!mbFuseSets) {
        mnSetLimit = orbhip_set_limit(mpCtx, FUSE_SETS);
        mbFuseSets = true;
    }
    *setKey = set_key_of(pKF);
    return hipdetail::ensure_set(mpCtx, *setKey, *pKF, pKF->mvKeysUn, pKF->mnMinX, pKF->mnMinY, pKF->mfGridElementWidthInv,
                                 pKF->mfGridElementHeightInv, NULL);
}

void LocalMapSearch::FuseEdits::Remember(MapPoint *surv)
{
    if (survivors.count(surv)) return;   // (nothing has changed its descriptor since the device call, or it would be here)
    const cv::Mat d = surv->GetDescriptor();
    survivors[surv].assign(d.ptr(0), d.ptr(0) + 32);
}

bool LocalMapSearch::FuseEdits::ChangedSince(MapPoint *pMP) const
{
    const std::map<MapPoint *, std::vector<unsigned char> >::const_iterator it = survivors.find(pMP);
    if (it == survivors.end()) return false;
    const cv::Mat d = pMP->GetDescriptor();
    return memcmp(d.ptr(0), it->second.data(), 32) != 0;
}

void LocalMapSearch::FuseEdits::Replace(MapPoint *dead, MapPoint *surv)
{
    Remember(surv);
    const std::map<KeyFrame *, size_t> obs = dead->GetObservations();
    dead->Replace(surv);
    for (std::map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) entries.insert(std::make_pair(it->first, it->second));
    flags.insert(dead);
    put.insert(surv);   // its descriptor (ComputeDistinctiveDescriptors, ref: src/MapPoint.cc:227) and flags
}

bool localmapdetail::research_survivors(orbhip_ctx *ctx, const std::vector<int> &redo, const orbhip_proj_query *Q, const std::vector<MapPoint *> &vpMPs,
                                        uint64_t setKey, const float *uRight, const float *invLevelSigma2, int nlevels, int32_t *bestIdx,
                                        int32_t *bestDist, ResearchBuffers &b)
{
    const int m = (int)redo.size();
    b.q.resize(m), b.qdesc.resize((size_t)m * 32), b.idx.resize(m), b.dist.resize(m);
    for (int k = 0; k < m; k++) {
        b.q[k] = Q[redo[k]];
        const cv::Mat d = vpMPs[redo[k]]->GetDescriptor();
        memcpy(&b.qdesc[(size_t)k * 32], d.ptr(0), 32);
    }
    if (orbhip_window_best_set(ctx, setKey, uRight, invLevelSigma2, nlevels, b.q.data(), b.qdesc.data(), m, b.idx.data(), b.dist.data()) != ORBHIP_OK) return false;
    for (int k = 0; k < m; k++) bestIdx[redo[k]] = b.idx[k], bestDist[redo[k]] = b.dist[k];
    return true;
}

// ref: src/ORBmatcher.cc:951-972 over the results of one target, in the caller's order.  An edit can change what a later point
// sees -- a point replaced a moment ago is bad now, a feature claimed a moment ago holds a point now, a point that survived a
// Replace is in more key frames now -- so isBad(), IsInKeyFrame() and the feature are read here, not before the search.
int LocalMapSearch::ApplyFuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMPs, const int32_t *bestIdx, const int32_t *bestDist,
                              FuseEdits &edits)
{
    const int nFeat = (int)pKF->GetMapPointMatches().size();
    int fused = 0;
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *cand = vpMPs[i];
        if (!cand || cand->isBad() || cand->IsInKeyFrame(pKF)) continue;          // ref: :844-848
        if (bestIdx[i] < 0 || bestIdx[i] >= nFeat || bestDist[i] > TH_LOW) continue;
        const size_t feat = (size_t)bestIdx[i];
        if (MapPoint *held = pKF->GetMapPoint(feat)) {
            if (!held->isBad()) {
                MapPoint *dead = held->Observations() > cand->Observations() ? cand : held, *surv = dead == cand ? held : cand;
                edits.Replace(dead, surv);
            }
        } else {
            cand->AddObservation(pKF, feat);
            pKF->AddMapPoint(cand, feat);
            edits.entries.insert(std::make_pair(pKF, feat));
            edits.flags.insert(cand);
        }
        fused++;      // (counted also when the held point was bad and nothing changed, as in the reference)
    }
    return fused;
}

// What FlushFuse and FlushLoop share.  The store as the objects are now: survivors' descriptors and flags, the flags of every other point
// an edit touched.  Then the row entries an edit may have changed, for the caller to write: key frame -> (indices, point keys).  Uses up the edits.
bool LocalMapSearch::TakeFuseEdits(FuseEdits &edits, FuseRows &rows)
{
    bool ok = edits.put.empty() || PutLocked(std::vector<MapPoint *>(edits.put.begin(), edits.put.end()));
    std::vector<MapPoint *> others;   // (the Put has carried the survivors' flags)
    for (std::set<MapPoint *>::const_iterator it = edits.flags.begin(); it != edits.flags.end(); ++it)
        if (!edits.put.count(*it) && Known(*it)) others.push_back(*it);
    ok = UpdateFlagsLocked(others.data(), others.size(), "LocalMapSearch::Fuse (orbhip_map_update_flags)") && ok;
    for (std::set<std::pair<KeyFrame *, size_t> >::const_iterator it = edits.entries.begin(); it != edits.entries.end(); ++it) {
        KeyFrame *kf = it->first;
        if (!HasRow(kf)) continue;
        MapPoint *p = kf->GetMapPoint(it->second);
        const bool named = p && Known(p) && p->GetIndexInKeyFrame(kf) == (int)it->second;   // PutKeyFrame's rule
        rows[key_of(kf)].first.push_back((int32_t)it->second);
        rows[key_of(kf)].second.push_back(named ? key_of(p) : 0);
    }
    edits.put.clear(), edits.flags.clear(), edits.entries.clear();
    return ok;
}

// the store and the table as the objects are now
bool LocalMapSearch::FlushFuse(FuseEdits &edits)
{
    FuseRows rows;
    bool ok = TakeFuseEdits(edits, rows);
    for (FuseRows::const_iterator it = rows.begin(); it != rows.end(); ++it)
        if (orbhip_map_kf_set(mpCtx, it->first, (int)it->second.first.size(), it->second.first.data(), it->second.second.data()) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::Fuse (orbhip_map_kf_set)", orbhip_last_error(mpCtx));
            ok = false;
        }
    return ok;
}

std::vector<int> LocalMapSearch::FuseInTargets(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const int K = (int)vpTargetKFs.size();
    std::vector<int> nFused(K, 0);
    if (K == 0 || !EnsureKeyFrames()) return nFused;
    const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();     // ref: src/LocalMapping.cc:2551 (one copy for all targets)
    const int n = (int)vpMPs.size();
    if (n == 0) return nFused;
    if (!EnsureRow(pKF)) return nFused;
    for (int k = 0; k < K; k++)
        if (!has_pyramid(vpTargetKFs[k]))
            return hipdetail::Fail("LocalMapSearch::FuseInTargets", "a target has no scale pyramid (mnScaleLevels, mvScaleFactors, mvInvLevelSigma2)"), nFused;
    // later calls read the list as it was: the row of pKF changes when one of its points is replaced
    std::vector<uint64_t> snapshot;
    if (K > FUSE_CHUNK) {
        snapshot.assign(n, 0);
        for (int i = 0; i < n; i++)
            if (vpMPs[i] && Known(vpMPs[i]) && vpMPs[i]->GetIndexInKeyFrame(pKF) == i) snapshot[i] = key_of(vpMPs[i]);
    }
    FuseEdits edits;
    bool snapshotPut = false;
    std::vector<orbhip_fuse_target> targets;
    std::vector<uint8_t> skip;
    std::vector<float> uRight;
    std::vector<orbhip_proj_query> queries;
    std::vector<int32_t> bestIdx, bestDist, nActive;
    std::vector<int> redo;
    localmapdetail::ResearchBuffers again;
    for (int start = 0; start < K; start += FUSE_CHUNK) {
        const int cnt = std::min(FUSE_CHUNK, K - start);
        uint64_t rowKey = key_of(pKF);
        if (start > 0) {
            if (!FlushFuse(edits)) return nFused;
            edits.survivors.clear();                          // the store has their descriptors now
            if (!snapshotPut && orbhip_map_kf_put(mpCtx, SNAPSHOT_ROW, n, snapshot.data()) != ORBHIP_OK)
                return hipdetail::Fail("LocalMapSearch::FuseInTargets (orbhip_map_kf_put)", orbhip_last_error(mpCtx)), nFused;
            snapshotPut = true;
            rowKey = SNAPSHOT_ROW;
        }
        targets.resize(cnt);
        skip.assign((size_t)cnt * n, 0);
        uRight.clear();
        bool anyStereo = false;
        std::vector<size_t> urAt(cnt);
        for (int j = 0; j < cnt; j++) {
            KeyFrame *pKFi = vpTargetKFs[start + j];
            uint64_t setKey = 0;
            if (!EnsureFuseSet(pKFi, &setKey))
                return hipdetail::Fail("LocalMapSearch::FuseInTargets (key frame set)", orbhip_last_error(mpCtx)), nFused;
            fill_target(pKFi, setKey, th, &targets[j]);
            for (int i = 0; i < n; i++)
                if (vpMPs[i] && vpMPs[i]->IsInKeyFrame(pKFi)) skip[(size_t)j * n + i] = 1;     // ref: src/ORBmatcher.cc:847
            urAt[j] = uRight.size();
            if (is_stereo(pKFi)) {
                anyStereo = true;
                uRight.insert(uRight.end(), pKFi->mvuRight.begin(), pKFi->mvuRight.end());
            } else
                uRight.insert(uRight.end(), pKFi->mvKeysUn.size(), -1.0f);                     // a monocular key frame among stereo ones
        }
        const size_t total = (size_t)cnt * n;
        queries.resize(total), bestIdx.resize(total), bestDist.resize(total), nActive.resize(cnt);
        if (orbhip_fuse_row(mpCtx, rowKey, targets.data(), cnt, skip.data(), anyStereo ? uRight.data() : NULL, queries.data(), bestIdx.data(),
                            bestDist.data(), nActive.data()) != ORBHIP_OK)
            return hipdetail::Fail("LocalMapSearch::FuseInTargets", orbhip_last_error(mpCtx)), nFused;
        for (int j = 0; j < cnt; j++) {
            KeyFrame *pKFi = vpTargetKFs[start + j];
            const orbhip_proj_query *Q = &queries[(size_t)j * n];
            // points whose descriptor changed since the call (they survived a Replace in an earlier target): their windows are
            // what they were, their best feature may not be.  (SearchAndFuse asks more of a point, and searches without uRight and sigmas)
            redo.clear();
            for (int i = 0; i < n && !edits.survivors.empty(); i++)
                if ((Q[i].flags & ORBHIP_Q_ACTIVE) && vpMPs[i] && edits.ChangedSince(vpMPs[i])) redo.push_back(i);
            int32_t *bi = &bestIdx[(size_t)j * n], *bd = &bestDist[(size_t)j * n];
            if (!redo.empty() && !localmapdetail::research_survivors(mpCtx, redo, Q, vpMPs, targets[j].set_key, anyStereo ? &uRight[urAt[j]] : NULL,
                                                                     targets[j].inv_level_sigma2, pKFi->mnScaleLevels, bi, bd, again))
                return hipdetail::Fail("LocalMapSearch::FuseInTargets (orbhip_window_best_set)", orbhip_last_error(mpCtx)), nFused;
            nFused[start + j] = ApplyFuse(pKFi, vpMPs, bi, bd, edits);
        }
    }
    FlushFuse(edits);
    if (snapshotPut) orbhip_map_kf_erase(mpCtx, SNAPSHOT_ROW);
    return nFused;
}

int LocalMapSearch::FuseCandidates(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (vpTargetKFs.empty() || !EnsureKeyFrames()) return 0;
    if (!has_pyramid(pKF))
        return hipdetail::Fail("LocalMapSearch::FuseCandidates", "the key frame has no scale pyramid (mnScaleLevels, mvScaleFactors, mvInvLevelSigma2)"), 0;
    if (!EnsureRow(pKF)) return 0;
    for (size_t k = 0; k < vpTargetKFs.size(); k++)
        if (!EnsureRow(vpTargetKFs[k])) return 0;
    std::vector<uint64_t> kfKeys;
    CollectKeys(vpTargetKFs, kfKeys);
    uint64_t setKey = 0;
    if (!EnsureFuseSet(pKF, &setKey)) return hipdetail::Fail("LocalMapSearch::FuseCandidates (key frame set)", orbhip_last_error(mpCtx)), 0;
    orbhip_fuse_target target;
    fill_target(pKF, setKey, th, &target);
    int ncand = 0, nActive = 0;
    std::vector<uint64_t> keys;
    std::vector<int32_t> bestIdx, bestDist;
    const int rc = call_with_room(room_for(mnLastCandidates, mPointOf.size()), &ncand, [&](int cap, size_t room) {
        keys.resize(room), bestIdx.resize(room), bestDist.resize(room);
        return orbhip_fuse_collect(mpCtx, &target, key_of(pKF), (int)kfKeys.size(), kfKeys.data(), is_stereo(pKF) ? pKF->mvuRight.data() : NULL,
                                   keys.data(), cap, &ncand, NULL, bestIdx.data(), bestDist.data(), &nActive);
    });
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::FuseCandidates", orbhip_last_error(mpCtx)), 0;
    mnLastCandidates = ncand;
    std::vector<MapPoint *> vpCandidates;
    PointsOf(keys.data(), ncand, vpCandidates);   // ref: src/LocalMapping.cc:2563-2580, element for element
    FuseEdits edits;
    const int fused = ApplyFuse(pKF, vpCandidates, bestIdx.data(), bestDist.data(), edits);
    FlushFuse(edits);
    return fused;
}

}  // namespace ORB_SLAM2
