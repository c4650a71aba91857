// LocalMapBowCand.cc -- LocalMapSearch::SearchByBoWCandidates (include/orbhip/LocalMap.h): ORBmatcher::SearchByBoW of one frame or
// key frame against every candidate key frame of Tracking::Relocalization (ref: src/Tracking.cc:2595-2616) and
// LoopClosing::ComputeSim3 (ref: src/LoopClosing.cc:304-332) as one orbhip_search_by_bow_candidates call on resident sets and rows
// (DESIGN.md section 21).  The matches come back as feature indices and are turned into MapPoint* from GetMapPointMatches() here; a
// key frame the store cannot speak for goes the way that existed before: ORBmatcher::SearchByBoW.  A file of its own: programs
// that link the other LocalMap*.cc files alone do not need the entry point.
#include <algorithm>

#include "LocalMapDetail.h"
#include "../MatcherDetail.h"
#include "ORBmatcher.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::key_of;

namespace
{
const int TH_LOW = 50;   // ORBmatcher::TH_LOW

// PnPsolver::PnPsolver's walk and the mvMaxError loop on the host (ref: src/PnPsolver.cc:78-101, :154-156)
void host_setup(Frame &F, const std::vector<MapPoint *> &vpMapPointMatches, float th2, RelocCorrespondences &out)
{
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        const cv::KeyPoint &kp = F.mvKeysUn[i];
        out.mvP2D.push_back(kp.pt);
        out.mvMaxError.push_back(F.mvLevelSigma2[kp.octave] * th2);
        const cv::Mat Pos = pMP->GetWorldPos();
        out.mvP3Dw.push_back(cv::Point3f(Pos.at<float>(0, 0), Pos.at<float>(1, 0), Pos.at<float>(2, 0)));
        out.mvKeyPointIndices.push_back(i);
    }
}
}  // namespace

// Can the table speak for pKF?  Every non-NULL, non-bad point known to the store (the rule of UpdateConnections); then its row is
// put when it has none and its features become a resident set.  false: the host way.
bool LocalMapSearch::ResidentKeyFrame(KeyFrame *pKF, uint64_t *setKey)
{
    const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();
    if ((int)vpMPs.size() != pKF->mDescriptors.rows || vpMPs.empty()) return false;
    if (!AllKnown(vpMPs) || !EnsureRow(pKF)) return false;
    if (!EnsureFuseSet(pKF, setKey)) return hipdetail::Fail("LocalMapSearch::SearchByBoWCandidates (key frame set)", orbhip_last_error(mpCtx)), false;
    return true;
}

// Which way each candidate goes: -2 nothing to do (NULL or bad; ref: src/Tracking.cc:2598-2599), -1 the host way (no device, or the
// table cannot speak for it), >= 0 its place among the device candidates, where who[place] is its index in the caller's vector.
void LocalMapSearch::SortCandidates(const std::vector<KeyFrame *> &vpKFs, bool device, std::vector<int> &way,
                                    std::vector<orbhip_bow_candidate> &cand, std::vector<size_t> &who)
{
    way.assign(vpKFs.size(), -1);
    for (size_t k = 0; k < vpKFs.size(); k++) {
        uint64_t setKey = 0;
        if (!vpKFs[k] || vpKFs[k]->isBad())
            way[k] = -2;
        else if (device && ResidentKeyFrame(vpKFs[k], &setKey)) {
            way[k] = (int)cand.size();
            const orbhip_bow_candidate c = {setKey, key_of(vpKFs[k])};
            cand.push_back(c);
            who.push_back(k);
        }
    }
}

void LocalMapSearch::SearchByBoWCandidates(const std::vector<KeyFrame *> &vpCandidateKFs, Frame &F,
                                           std::vector<std::vector<MapPoint *> > &vvpMapPointMatches, std::vector<int> &vnMatches,
                                           std::vector<RelocCorrespondences> *pvSetups, int minMatches, float th2, float nnratio, bool checkOri)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const size_t K = vpCandidateKFs.size();
    vvpMapPointMatches.assign(K, std::vector<MapPoint *>());
    vnMatches.assign(K, 0);
    if (pvSetups) pvSetups->assign(K, RelocCorrespondences());

    std::vector<int> way;
    std::vector<orbhip_bow_candidate> cand;
    std::vector<size_t> who;
    const bool gather = pvSetups != 0;
    uint64_t frameKey = (uint64_t)F.mnId + 1;
    bool device = F.N > 0 && EnsureKeyFrames() && (!gather || ((int)F.mvLevelSigma2.size() >= 1 && (int)F.mvLevelSigma2.size() <= 64));
    if (device && !hipdetail::ensure_set(mpCtx, frameKey, F, F.mvKeysUn, Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv,
                                         Frame::mfGridElementHeightInv, NULL)) {
        hipdetail::Fail("LocalMapSearch::SearchByBoWCandidates (frame set)", orbhip_last_error(mpCtx));
        device = false;
    }
    SortCandidates(vpCandidateKFs, device, way, cand, who);

    // ---- the device candidates, as many to a call as the set limit leaves room for beside the frame ----
    const int nF = F.N, chunk = std::max(1, mnSetLimit - 1);
    std::vector<int32_t> matches, nm, off, kpIdx, kfIdx;
    std::vector<float> P3, P2, me;
    for (size_t start = 0; start < cand.size(); start += (size_t)chunk) {
        const int cnt = (int)std::min(cand.size() - start, (size_t)chunk);
        // (with more than one chunk, a set put for a later candidate may have pushed out one of this chunk: made sure of again)
        const bool again = cand.size() > (size_t)chunk;
        bool ok = !again || hipdetail::ensure_set(mpCtx, frameKey, F, F.mvKeysUn, Frame::mnMinX, Frame::mnMinY, Frame::mfGridElementWidthInv,
                                                  Frame::mfGridElementHeightInv, NULL);
        for (int j = 0; j < cnt && ok && again; j++) {
            uint64_t setKey = 0;
            ok = EnsureFuseSet(vpCandidateKFs[who[start + j]], &setKey);
        }
        matches.assign((size_t)cnt * nF, -1), nm.assign(cnt, 0);
        int rc = ORBHIP_E_HIP, total = 0;
        if (ok && gather) {
            const int cap = cnt * nF;
            off.assign(cnt + 1, 0), kpIdx.resize(cap), kfIdx.resize(cap), P3.resize((size_t)cap * 3), P2.resize((size_t)cap * 2), me.resize(cap);
            rc = orbhip_search_by_bow_candidates(mpCtx, 0, frameKey, 0, &cand[start], cnt, TH_LOW, nnratio, checkOri ? 1 : 0, matches.data(),
                                                 nm.data(), minMatches, F.mvLevelSigma2.data(), (int)F.mvLevelSigma2.size(), th2, off.data(),
                                                 kpIdx.data(), kfIdx.data(), P3.data(), P2.data(), me.data(), cap, &total);
        } else if (ok)
            rc = orbhip_search_by_bow_candidates(mpCtx, 0, frameKey, 0, &cand[start], cnt, TH_LOW, nnratio, checkOri ? 1 : 0, matches.data(),
                                                 nm.data(), 0, NULL, 0, 0.f, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL);
        if (rc != ORBHIP_OK) {               // the answer stays right: these candidates go the host way
            hipdetail::Fail("LocalMapSearch::SearchByBoWCandidates", orbhip_last_error(mpCtx));
            for (int j = 0; j < cnt; j++) way[who[start + j]] = -1;
            continue;
        }
        for (int j = 0; j < cnt; j++) {
            const size_t k = who[start + j];
            const std::vector<MapPoint *> vpMPs = vpCandidateKFs[k]->GetMapPointMatches();
            std::vector<MapPoint *> &out = vvpMapPointMatches[k];
            out.assign(nF, static_cast<MapPoint *>(NULL));
            const int32_t *row = &matches[(size_t)j * nF];
            for (int i = 0; i < nF; i++)
                if (row[i] >= 0 && row[i] < (int)vpMPs.size()) out[i] = vpMPs[row[i]];
            vnMatches[k] = nm[j];
            BowCandCounts().device++;
            if (!gather) continue;
            RelocCorrespondences &S = (*pvSetups)[k];
            for (int t = off[j]; t < off[j + 1]; t++) {
                S.mvP2D.push_back(cv::Point2f(P2[2 * (size_t)t], P2[2 * (size_t)t + 1]));
                S.mvMaxError.push_back(me[t]);
                S.mvP3Dw.push_back(cv::Point3f(P3[3 * (size_t)t], P3[3 * (size_t)t + 1], P3[3 * (size_t)t + 2]));
                S.mvKeyPointIndices.push_back((size_t)kpIdx[t]);
            }
        }
    }

    // ---- the host way ----
    lock.unlock();                           // (ORBmatcher has a context of its own)
    for (size_t k = 0; k < K; k++) {
        if (way[k] != -1) continue;
        ORBmatcher matcher(nnratio, checkOri);
        vnMatches[k] = matcher.SearchByBoW(vpCandidateKFs[k], F, vvpMapPointMatches[k]);
        BowCandCounts().host++;
        if (gather && vnMatches[k] >= minMatches) host_setup(F, vvpMapPointMatches[k], th2, (*pvSetups)[k]);
    }
}

void LocalMapSearch::SearchByBoWCandidates(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCandidateKFs,
                                           std::vector<std::vector<MapPoint *> > &vvpMatches12, std::vector<int> &vnMatches, float nnratio,
                                           bool checkOri)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const size_t K = vpCandidateKFs.size();
    vvpMatches12.assign(K, std::vector<MapPoint *>());
    vnMatches.assign(K, 0);
    if (!pCurrentKF) return;

    std::vector<int> way;
    std::vector<orbhip_bow_candidate> cand;
    std::vector<size_t> who;
    uint64_t curSet = 0;
    const bool device = EnsureKeyFrames() && ResidentKeyFrame(pCurrentKF, &curSet);
    SortCandidates(vpCandidateKFs, device, way, cand, who);

    const int n1 = (int)pCurrentKF->GetMapPointMatches().size(), chunk = std::max(1, mnSetLimit - 1);
    std::vector<int32_t> matches, nm;
    for (size_t start = 0; start < cand.size(); start += (size_t)chunk) {
        const int cnt = (int)std::min(cand.size() - start, (size_t)chunk);
        const bool again = cand.size() > (size_t)chunk;   // (as above)
        bool ok = !again || EnsureFuseSet(pCurrentKF, &curSet);
        for (int j = 0; j < cnt && ok && again; j++) {
            uint64_t setKey = 0;
            ok = EnsureFuseSet(vpCandidateKFs[who[start + j]], &setKey);
        }
        matches.assign((size_t)cnt * n1, -1), nm.assign(cnt, 0);
        const int rc = !ok ? ORBHIP_E_HIP
                           : orbhip_search_by_bow_candidates(mpCtx, 1, curSet, key_of(pCurrentKF), &cand[start], cnt, TH_LOW, nnratio,
                                                             checkOri ? 1 : 0, matches.data(), nm.data(), 0, NULL, 0, 0.f, NULL, NULL, NULL, NULL,
                                                             NULL, NULL, 0, NULL);
        if (rc != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::SearchByBoWCandidates", orbhip_last_error(mpCtx));
            for (int j = 0; j < cnt; j++) way[who[start + j]] = -1;
            continue;
        }
        for (int j = 0; j < cnt; j++) {
            const size_t k = who[start + j];
            const std::vector<MapPoint *> vpMPs2 = vpCandidateKFs[k]->GetMapPointMatches();
            std::vector<MapPoint *> &out = vvpMatches12[k];
            out.assign(n1, static_cast<MapPoint *>(NULL));
            const int32_t *row = &matches[(size_t)j * n1];
            for (int i = 0; i < n1; i++)
                if (row[i] >= 0 && row[i] < (int)vpMPs2.size()) out[i] = vpMPs2[row[i]];      // ref: src/ORBmatcher.cc:602
            vnMatches[k] = nm[j];
            BowCandCounts().device++;
        }
    }

    lock.unlock();
    for (size_t k = 0; k < K; k++) {
        if (way[k] != -1) continue;
        ORBmatcher matcher(nnratio, checkOri);
        vnMatches[k] = matcher.SearchByBoW(pCurrentKF, vpCandidateKFs[k], vvpMatches12[k]);
        BowCandCounts().host++;
    }
}

}  // namespace ORB_SLAM2
