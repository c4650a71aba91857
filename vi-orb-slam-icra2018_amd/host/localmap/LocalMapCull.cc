// LocalMapCull.cc -- LocalMapSearch::CullCounts and KeyFrameCulled (include/orbhip/LocalMap.h): the counting loop of
// LocalMapping::KeyFrameCulling and of the fork's KeyFrameCullingForMonoVI (ref: src/LocalMapping.cc:2705-2753, :1533-1581; DESIGN.md
// section 22) for a batch of key frames in one orbhip_map_cull call on the resident key-frame table.  The call counts on the map as
// it is; the sequence -- one cull at a time, the candidates behind it counted again -- is kept by the template KeyFrameCulling in
// the header.  A key frame the table cannot speak for goes the way that existed before: the loop on the objects.  A file of its
// own: programs that link the other LocalMap*.cc files alone do not need the entry points.
#include <algorithm>
#include <map>
#include <set>

#include "LocalMapDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::key_of;

namespace
{
const int kThObs = 3;   // ref: src/LocalMapping.cc:2711

inline bool far_point(KeyFrame *pKF, size_t i)   // ref: :2722
{
    return i < pKF->mvDepth.size() && (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0);
}

// the reference's loop for one key frame, on the objects
LocalMapSearch::CullCount host_count(KeyFrame *pKF, bool bMonocular)
{
    const std::vector<MapPoint *> vpMapPoints = pKF->GetMapPointMatches();
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPoints[i];
        if (!pMP || pMP->isBad()) continue;
        if (!bMonocular && far_point(pKF, i)) continue;
        nMPs++;
        if (pMP->Observations() <= kThObs) continue;
        const int scaleLevel = pKF->mvKeysUn[i].octave;
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        int nObs = 0;
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
            KeyFrame *pKFi = mit->first;
            if (pKFi == pKF) continue;
            if (pKFi->mvKeysUn[mit->second].octave <= scaleLevel + 1 && ++nObs >= kThObs) break;
        }
        if (nObs >= kThObs) nRedundantObservations++;
    }
    const LocalMapSearch::CullCount c = {nMPs, nRedundantObservations, nRedundantObservations > 0.9 * nMPs};
    return c;
}

// one byte per feature of the key frame's row: octave | stereo << 6 | far << 7 (include/orbhip.h); false: an octave outside 0..15
bool level_bytes(KeyFrame *pKF, std::vector<uint8_t> &bytes)
{
    const size_t n = pKF->GetMapPointMatches().size();
    for (size_t i = 0; i < n; i++) {
        const int octave = i < pKF->mvKeysUn.size() ? pKF->mvKeysUn[i].octave : 0;
        if (octave < 0 || octave > 15) return false;
        const bool stereo = i < pKF->mvuRight.size() && pKF->mvuRight[i] >= 0;
        bytes.push_back((uint8_t)(octave | (stereo ? 0x40 : 0) | (far_point(pKF, i) ? 0x80 : 0)));
    }
    return true;
}
}  // namespace

bool LocalMapSearch::CullCounts(const std::vector<KeyFrame *> &vpKFs, bool bMonocular, std::vector<CullCount> &vCounts)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EnsureKeyFrames()) return false;
    const size_t n = vpKFs.size();
    // which way each key frame goes; the rows the call needs
    std::vector<int> cand(n, -1);   // the key frame's position among the candidates, -1: the host way
    std::vector<uint64_t> keys;
    for (size_t k = 0; k < n; k++) {
        KeyFrame *pKF = vpKFs[k];
        if (!pKF || pKF->isBad()) continue;   // (a bad key frame has no row and gets none)
        if (!AllKnown(pKF->GetMapPointMatches())) continue;   // this key frame goes the host way
        if (!EnsureRow(pKF)) return false;
        cand[k] = (int)keys.size();
        keys.push_back(key_of(pKF));
    }

    std::vector<orbhip_cull_count> counts(keys.size() ? keys.size() : 1);
    std::vector<uint8_t> redundant(counts.size(), 0);
    if (!keys.empty()) {
        // ---- the levels of the rows that have none yet: every live row is an observer ----
        std::vector<uint64_t> missing(mKeyFrameOf.size() ? mKeyFrameOf.size() : 1);
        int nMissing = 0;
        if (orbhip_map_kf_levels_missing(mpCtx, missing.data(), (int)missing.size(), &nMissing) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::CullCounts (orbhip_map_kf_levels_missing)", orbhip_last_error(mpCtx));
            return false;
        }
        if (nMissing > 0) {
            std::vector<int32_t> off(1, 0);
            std::vector<uint8_t> bytes;
            for (int q = 0; q < nMissing; q++) {
                KeyFrame *pKF = KeyFrameOf(missing[q]);
                if (!pKF || !level_bytes(pKF, bytes)) {
                    hipdetail::Fail("LocalMapSearch::CullCounts", "a row of the table without its key frame, or an octave outside 0..15");
                    return false;
                }
                off.push_back((int32_t)bytes.size());
            }
            if (bytes.empty()) bytes.push_back(0);
            if (orbhip_map_kf_levels(mpCtx, nMissing, missing.data(), off.data(), bytes.data()) != ORBHIP_OK) {
                hipdetail::Fail("LocalMapSearch::CullCounts (orbhip_map_kf_levels)", orbhip_last_error(mpCtx));
                return false;
            }
        }
        // ---- the counts of every candidate: one device call ----
        if (orbhip_map_cull(mpCtx, (int)keys.size(), keys.data(), bMonocular ? 1 : 0, kThObs, counts.data(), redundant.data(), NULL) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::CullCounts (orbhip_map_cull)", orbhip_last_error(mpCtx));
            return false;
        }
    }

    vCounts.resize(n);
    for (size_t k = 0; k < n; k++) {
        if (!vpKFs[k]) {
            const CullCount none = {0, 0, false};
            vCounts[k] = none;
        } else if (cand[k] < 0) {
            vCounts[k] = host_count(vpKFs[k], bMonocular);
            CullWayCounts().host++;
        } else {
            const CullCount c = {counts[cand[k]].n_mps, counts[cand[k]].n_redundant, redundant[cand[k]] != 0};
            vCounts[k] = c;
            CullWayCounts().device++;
        }
    }
    return true;
}

void LocalMapSearch::KeyFrameCulled(KeyFrame *pKF, const std::vector<MapPoint *> &vpItsPoints)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!EraseKeyFrameLocked(pKF, "LocalMapSearch::KeyFrameCulled (orbhip_map_kf_erase)")) return;
    // the points EraseObservation left with two observations or fewer turned bad: their entries in the other rows resolve no longer
    std::set<uint64_t> seen;
    std::vector<MapPoint *> turnedBad;
    for (size_t i = 0; i < vpItsPoints.size(); i++) {
        MapPoint *pMP = vpItsPoints[i];
        if (pMP && pMP->isBad() && Known(pMP) && seen.insert(key_of(pMP)).second) turnedBad.push_back(pMP);
    }
    UpdateFlagsLocked(turnedBad.data(), turnedBad.size(), "LocalMapSearch::KeyFrameCulled (orbhip_map_update_flags)");
}

}  // namespace ORB_SLAM2
