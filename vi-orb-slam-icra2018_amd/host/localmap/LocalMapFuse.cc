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

using localmapdetail::fill_target;
using localmapdetail::flags_of;
using localmapdetail::has_pyramid;
using localmapdetail::key_of;
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
                const std::map<KeyFrame *, size_t> obs = dead->GetObservations();
                if (!edits.survivors.count(surv)) {   // (nothing has changed its descriptor since the device call, or it would be here)
                    const cv::Mat d = surv->GetDescriptor();
                    edits.survivors[surv].assign(d.ptr(0), d.ptr(0) + 32);
                }
                dead->Replace(surv);
                for (std::map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it)
                    edits.entries.insert(std::make_pair(it->first, it->second));
                edits.flags.insert(dead);
                edits.put.insert(surv);           // its descriptor (ComputeDistinctiveDescriptors, ref: src/MapPoint.cc:227) and flags
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

// the store as the objects are now: survivors' descriptors and flags, the flags of every other point an edit touched
bool LocalMapSearch::FlushFusePoints(FuseEdits &edits)
{
    bool ok = true;
    if (!edits.put.empty()) ok = PutLocked(std::vector<MapPoint *>(edits.put.begin(), edits.put.end())) && ok;
    std::vector<uint64_t> keys;
    std::vector<uint8_t> fl;
    for (std::set<MapPoint *>::const_iterator it = edits.flags.begin(); it != edits.flags.end(); ++it) {
        if (edits.put.count(*it) || !mPointOf.count(key_of(*it))) continue;
        keys.push_back(key_of(*it));
        fl.push_back(flags_of(*it));
    }
    if (!keys.empty() && orbhip_map_update_flags(mpCtx, (int)keys.size(), keys.data(), fl.data()) != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch::Fuse (orbhip_map_update_flags)", orbhip_last_error(mpCtx));
        ok = false;
    }
    return ok;
}

// the row entries an edit may have changed, as the objects hold them now: key frame -> (indices, point keys)
void LocalMapSearch::FuseRowEdits(const FuseEdits &edits, FuseRows &rows)
{
    for (std::set<std::pair<KeyFrame *, size_t> >::const_iterator it = edits.entries.begin(); it != edits.entries.end(); ++it) {
        KeyFrame *kf = it->first;
        if (!mKeyFrameOf.count(key_of(kf))) continue;
        MapPoint *p = kf->GetMapPoint(it->second);
        const bool named = p && mPointOf.count(key_of(p)) && p->GetIndexInKeyFrame(kf) == (int)it->second;   // PutKeyFrame's rule
        rows[key_of(kf)].first.push_back((int32_t)it->second);
        rows[key_of(kf)].second.push_back(named ? key_of(p) : 0);
    }
}

// the store and the table as the objects are now
bool LocalMapSearch::FlushFuse(FuseEdits &edits)
{
    bool ok = FlushFusePoints(edits);
    FuseRows rows;
    FuseRowEdits(edits, rows);
    for (FuseRows::const_iterator it = rows.begin(); it != rows.end(); ++it)
        if (orbhip_map_kf_set(mpCtx, it->first, (int)it->second.first.size(), it->second.first.data(), it->second.second.data()) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::Fuse (orbhip_map_kf_set)", orbhip_last_error(mpCtx));
            ok = false;
        }
    edits.put.clear(), edits.flags.clear(), edits.entries.clear();
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
    if (!mKeyFrameOf.count(key_of(pKF)) && !PutKeyFrameLocked(pKF)) return nFused;
    for (int k = 0; k < K; k++)
        if (!has_pyramid(vpTargetKFs[k]))
            return hipdetail::Fail("LocalMapSearch::FuseInTargets", "a target has no scale pyramid (mnScaleLevels, mvScaleFactors, mvInvLevelSigma2)"), nFused;
    // later calls read the list as it was: the row of pKF changes when one of its points is replaced
    std::vector<uint64_t> snapshot;
    if (K > FUSE_CHUNK) {
        snapshot.assign(n, 0);
        for (int i = 0; i < n; i++)
            if (vpMPs[i] && mPointOf.count(key_of(vpMPs[i])) && vpMPs[i]->GetIndexInKeyFrame(pKF) == i) snapshot[i] = key_of(vpMPs[i]);
    }
    FuseEdits edits;
    bool snapshotPut = false;
    std::vector<orbhip_fuse_target> targets;
    std::vector<uint8_t> skip;
    std::vector<float> uRight;
    std::vector<orbhip_proj_query> queries, q;
    std::vector<int32_t> bestIdx, bestDist, nActive, rbi, rbd;
    std::vector<uint8_t> qdesc;
    std::vector<int> redo;
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
            // what they were, their best feature may not be
            redo.clear();
            for (int i = 0; i < n && !edits.survivors.empty(); i++) {
                if (!(Q[i].flags & ORBHIP_Q_ACTIVE) || !vpMPs[i]) continue;
                std::map<MapPoint *, std::vector<unsigned char> >::const_iterator it = edits.survivors.find(vpMPs[i]);
                if (it == edits.survivors.end()) continue;
                const cv::Mat d = vpMPs[i]->GetDescriptor();
                if (memcmp(d.ptr(0), it->second.data(), 32) != 0) redo.push_back(i);
            }
            if (!redo.empty()) {
                const int m = (int)redo.size();
                q.resize(m), qdesc.resize((size_t)m * 32), rbi.resize(m), rbd.resize(m);
                for (int k = 0; k < m; k++) {
                    q[k] = Q[redo[k]];
                    const cv::Mat d = vpMPs[redo[k]]->GetDescriptor();
                    memcpy(&qdesc[(size_t)k * 32], d.ptr(0), 32);
                }
                if (orbhip_window_best_set(mpCtx, targets[j].set_key, anyStereo ? &uRight[urAt[j]] : NULL, targets[j].inv_level_sigma2,
                                           pKFi->mnScaleLevels, q.data(), qdesc.data(), m, rbi.data(), rbd.data()) != ORBHIP_OK)
                    return hipdetail::Fail("LocalMapSearch::FuseInTargets (orbhip_window_best_set)", orbhip_last_error(mpCtx)), nFused;
                for (int k = 0; k < m; k++) bestIdx[(size_t)j * n + redo[k]] = rbi[k], bestDist[(size_t)j * n + redo[k]] = rbd[k];
            }
            nFused[start + j] = ApplyFuse(pKFi, vpMPs, &bestIdx[(size_t)j * n], &bestDist[(size_t)j * n], edits);
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
    if (!mKeyFrameOf.count(key_of(pKF)) && !PutKeyFrameLocked(pKF)) return 0;
    for (size_t k = 0; k < vpTargetKFs.size(); k++)
        if (!mKeyFrameOf.count(key_of(vpTargetKFs[k])) && !PutKeyFrameLocked(vpTargetKFs[k])) return 0;
    std::vector<uint64_t> kfKeys;
    CollectKeys(vpTargetKFs, kfKeys);
    uint64_t setKey = 0;
    if (!EnsureFuseSet(pKF, &setKey)) return hipdetail::Fail("LocalMapSearch::FuseCandidates (key frame set)", orbhip_last_error(mpCtx)), 0;
    orbhip_fuse_target target;
    fill_target(pKF, setKey, th, &target);
    int cap = (int)std::min(mPointOf.size(), mnLastCandidates + mnLastCandidates / 4 + 256), ncand = 0, nActive = 0;
    std::vector<uint64_t> keys;
    std::vector<int32_t> bestIdx, bestDist;
    for (;;) {   // the list is a function of the map, never of the room: too little room, and the call is made again with enough
        keys.resize(cap > 0 ? cap : 1), bestIdx.resize(cap > 0 ? cap : 1), bestDist.resize(cap > 0 ? cap : 1);
        const int rc = orbhip_fuse_collect(mpCtx, &target, key_of(pKF), (int)kfKeys.size(), kfKeys.data(),
                                           is_stereo(pKF) ? pKF->mvuRight.data() : NULL, keys.data(), cap, &ncand, NULL, bestIdx.data(),
                                           bestDist.data(), &nActive);
        if (rc == ORBHIP_E_CAPACITY && ncand > cap) {
            cap = ncand;
            continue;
        }
        if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::FuseCandidates", orbhip_last_error(mpCtx)), 0;
        break;
    }
    mnLastCandidates = ncand;
    std::vector<MapPoint *> vpCandidates(ncand, static_cast<MapPoint *>(NULL));   // ref: src/LocalMapping.cc:2563-2580, element for element
    for (int k = 0; k < ncand; k++) {
        std::unordered_map<uint64_t, MapPoint *>::iterator it = mPointOf.find(keys[k]);
        if (it != mPointOf.end()) vpCandidates[k] = it->second;
    }
    FuseEdits edits;
    const int fused = ApplyFuse(pKF, vpCandidates, bestIdx.data(), bestDist.data(), edits);
    FlushFuse(edits);
    return fused;
}

}  // namespace ORB_SLAM2
