// LocalMapCovis.cc -- LocalMapSearch::UpdateConnections (include/orbhip/LocalMap.h): KeyFrame::UpdateConnections for a batch of key
// frames (ref: src/KeyFrame.cc:731-843; the call sites src/LocalMapping.cc:2155, :2593 and src/LoopClosing.cc:567, :606;
// DESIGN.md section 20).  One orbhip_map_covis call counts the shared points of every key frame of the batch on the resident
// key-frame table and orders the links; the results are applied to the caller's KeyFrame objects in the vector's order, as
// sequential calls of the method would.  A key frame the table cannot speak for goes the way that existed before: the method
// itself.  A file of its own: programs that link the other LocalMap*.cc files alone do not need the entry point.
#include <algorithm>
#include <map>
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
const int kCovisTh = 15;   // ref: src/KeyFrame.cc:780

// LoopConnections[pKF] before the two erase loops: the key frames of mConnectedKeyFrameWeights
std::set<KeyFrame *> connected_set(KeyFrame *pKF)
{
#ifdef ORBHIP_WITH_REFERENCE_HEADERS
    return pKF->GetConnectedKeyFrames();
#else
    std::set<KeyFrame *> s;   // (slamlite.h's GetConnectedKeyFrames reads the ordered vector, which a caller may have filled by hand)
    for (std::map<KeyFrame *, int>::const_iterator it = pKF->mConnectedKeyFrameWeights.begin(); it != pKF->mConnectedKeyFrameWeights.end(); ++it)
        s.insert(it->first);
    return s;
#endif
}
}  // namespace

void LocalMapSearch::UpdateConnections(KeyFrame *pKF) { UpdateConnections(std::vector<KeyFrame *>(1, pKF)); }

void LocalMapSearch::UpdateConnections(const std::vector<KeyFrame *> &vpKFs, std::map<KeyFrame *, std::set<KeyFrame *> > *pLoopConnections,
                                       const std::vector<KeyFrame *> *pvpExclude)
{
    std::unique_lock<std::mutex> lock(mMutex);
    const size_t n = vpKFs.size();
    // which way each key frame goes; the rows the call needs
    std::vector<int> query(n, -1);   // the key frame's position among the queries, -1: the host way
    std::vector<uint64_t> keys;
    if (EnsureKeyFrames()) {
        for (size_t k = 0; k < n; k++) {
            KeyFrame *pKF = vpKFs[k];
            if (!pKF) continue;
            if (!AllKnown(pKF->GetMapPointMatches()) || !EnsureRow(pKF)) continue;   // this key frame goes the host way
            query[k] = (int)keys.size();
            keys.push_back(key_of(pKF));
        }
    }

    // ---- the counts and the ordered links of every query: one device call ----
    const int nq = (int)keys.size();
    std::vector<int32_t> off(nq + 1, 0), nord(nq > 0 ? nq : 1, 0), weights, order;
    std::vector<uint64_t> nbr;
    if (nq > 0) {
        int total = 0;
        const int rc = call_with_room(nq * room_for(mnLastLinks, mKeyFrameOf.size(), 16), &total, [&](int cap, size_t room) {   // 16 to spare per query
            nbr.resize(room), weights.resize(room), order.resize(room);
            return orbhip_map_covis(mpCtx, nq, keys.data(), kCovisTh, off.data(), nbr.data(), weights.data(), order.data(), nord.data(), cap, &total);
        });
        if (rc != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::UpdateConnections (orbhip_map_covis)", orbhip_last_error(mpCtx));
            std::fill(query.begin(), query.end(), -1);   // the graph stays right: every key frame goes the host way
        }
        mnLastLinks = ((size_t)total + nq - 1) / nq;
    }

    // ---- applied in the vector's order ----
    for (size_t k = 0; k < n; k++) {
        KeyFrame *pKF = vpKFs[k];
        if (!pKF) continue;
        std::vector<KeyFrame *> vpPrevious;
        if (pLoopConnections) vpPrevious = pKF->GetVectorCovisibleKeyFrames();
        if (query[k] < 0) {
            pKF->UpdateConnections();
            CovisCounts().host++;
        } else {
            CovisCounts().device++;
            const int a = off[query[k]], b = off[query[k] + 1];
            std::map<KeyFrame *, int> KFcounter;
            std::vector<KeyFrame *> seg(b - a, static_cast<KeyFrame *>(NULL));
            for (int i = a; i < b; i++) {
                KeyFrame *pNbr = KeyFrameOf(nbr[i]);
                if (!pNbr) continue;
                seg[i - a] = pNbr;
                KFcounter[pNbr] = weights[i];
            }
            if (!KFcounter.empty()) {   // (empty: the reference returns before it touches anything)
                std::vector<KeyFrame *> vpOrdered;
                std::vector<int> vWeights;
                for (int r = 0; r < nord[query[k]]; r++) {
                    const int i = order[a + r];
                    if (i < 0 || i >= b - a || !seg[i]) continue;
                    seg[i]->AddConnection(pKF, weights[a + i]);
                    vpOrdered.push_back(seg[i]);
                    vWeights.push_back(weights[a + i]);
                }
#ifdef ORBHIP_WITH_REFERENCE_HEADERS
                std::unique_lock<std::mutex> lockCon(pKF->mMutexConnections);
#endif
                pKF->mConnectedKeyFrameWeights = KFcounter;
                pKF->mvpOrderedConnectedKeyFrames = vpOrdered;
                pKF->mvOrderedWeights = vWeights;
                if (pKF->mbFirstConnection && pKF->mnId != 0 && !vpOrdered.empty()) {
                    pKF->mpParent = vpOrdered.front();
                    pKF->mpParent->AddChild(pKF);
                    pKF->mbFirstConnection = false;
                }
            }
        }
        if (pLoopConnections) {
            std::set<KeyFrame *> &s = (*pLoopConnections)[pKF];
            s = connected_set(pKF);
            for (size_t i = 0; i < vpPrevious.size(); i++) s.erase(vpPrevious[i]);
            if (pvpExclude)
                for (size_t i = 0; i < pvpExclude->size(); i++) s.erase((*pvpExclude)[i]);
        }
    }
}

}  // namespace ORB_SLAM2
