// LocalMapBA.cc -- LocalMapSearch::BuildLocalBA and BuildBAProblem (include/orbhip/LocalMap.h): what
// Optimizer::LocalBundleAdjustment forms before the solver sees a vertex (ref: src/Optimizer.cc:2772-2820 the local key frames,
// lLocalMapPoints and lFixedCameras, :2888 ff. one edge per observation) from one orbhip_map_ba_problem
// call on the resident key-frame table.  The call returns keys and indices; they become pointers here, at the moment of
// application, and the reference's stamps are left on the objects.  Nothing of the solver is touched.  A file of its own: programs
// that link the other LocalMap*.cc files alone do not need the entry point.
#include <algorithm>

#include "LocalMapDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::key_of;

bool LocalMapSearch::BuildLocalBA(KeyFrame *pKF, BAProblem &out)
{
    out = BAProblem();
    if (!pKF) return false;
    // Local KeyFrames: First Breath Search from Current Keyframe (ref: :2772-2784)
    std::vector<KeyFrame *> vpLocal(1, pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrame *> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (size_t i = 0; i < vNeighKFs.size(); i++) {
        KeyFrame *pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;   // (a bad neighbour is stamped local and not listed: it is never fixed)
        if (!pKFi->isBad()) vpLocal.push_back(pKFi);
    }
    std::unique_lock<std::mutex> lock(mMutex);
    return BuildBALocked(vpLocal, pKF->mnId, out);
}

bool LocalMapSearch::BuildBAProblem(const std::vector<KeyFrame *> &vpLocalKFs, BAProblem &out)
{
    out = BAProblem();
    std::vector<KeyFrame *> vpLocal;
    for (size_t i = 0; i < vpLocalKFs.size(); i++)
        if (vpLocalKFs[i] && !vpLocalKFs[i]->isBad()) vpLocal.push_back(vpLocalKFs[i]);
    if (vpLocal.empty()) return true;
    const unsigned long nStamp = vpLocal.back()->mnId;
    for (size_t i = 0; i < vpLocal.size(); i++) vpLocal[i]->mnBALocalForKF = nStamp;   // ref: :1002-1006
    std::unique_lock<std::mutex> lock(mMutex);
    return BuildBALocked(vpLocal, nStamp, out);
}

bool LocalMapSearch::BuildBALocked(const std::vector<KeyFrame *> &vpLocal, unsigned long nStamp, BAProblem &out)
{
    const char *who = "LocalMapSearch::BuildBAProblem (orbhip_map_ba_problem)";
    if (!EnsureKeyFrames()) return false;
    const int nkf = (int)vpLocal.size();
    std::vector<uint64_t> kfKeys(nkf);
    size_t mostPoints = 0;
    for (int k = 0; k < nkf; k++) {
        if (!HasRow(vpLocal[k])) return false;   // a local key frame without a row: the caller's loops (tests, does not put)
        kfKeys[k] = key_of(vpLocal[k]);
        mostPoints += (size_t)std::max(vpLocal[k]->N, 0);
    }
    // room: no call has more points than the local rows have features; edges and fixed key frames about as many as last time, and
    // the call is made again with the exact sizes when that was too little (the lists are a function of the map, never of the room)
    int capP = (int)std::min(mostPoints, mPointOf.size()), capE = (int)(mnLastBAEdges + mnLastBAEdges / 4 + 4096);
    int capF = (int)std::min(mKeyFrameOf.size(), mnLastBAFixed + mnLastBAFixed / 4 + 64);
    int np = 0, ne = 0, nf = 0;
    std::vector<uint64_t> ptKeys, fixedKeys;
    std::vector<int32_t> off;
    std::vector<orbhip_ba_edge> edges;
    // not call_with_room: three capacities, each raised to what the call reported, and one second call at the most
    for (int round = 0;; round++) {
        ptKeys.resize(capP > 0 ? capP : 1), fixedKeys.resize(capF > 0 ? capF : 1), off.resize((size_t)capP + 1), edges.resize(capE > 0 ? capE : 1);
        const int rc = orbhip_map_ba_problem(mpCtx, nkf, kfKeys.data(), ptKeys.data(), capP, &np, off.data(), edges.data(), capE, &ne,
                                             fixedKeys.data(), capF, &nf);
        if (rc == ORBHIP_E_CAPACITY && round == 0) {
            capP = std::max(capP, np), capE = std::max(capE, ne), capF = std::max(capF, nf);
            continue;
        }
        if (rc != ORBHIP_OK) return hipdetail::Fail(who, orbhip_last_error(mpCtx));
        break;
    }
    mnLastBAEdges = ne, mnLastBAFixed = nf;

    // ---- keys and indices become pointers; nothing is stamped before every one of them is known ----
    BAProblem P;
    P.vpLocalKFs = vpLocal;
    P.vpLocalMPs.resize(np), P.vpFixedKFs.resize(nf), P.vEdges.resize(ne);
    for (int j = 0; j < np; j++) {
        P.vpLocalMPs[j] = PointOf(ptKeys[j]);
        if (!P.vpLocalMPs[j]) return hipdetail::Fail(who, "a point of the store without its object");
    }
    for (int r = 0; r < nf; r++) {
        P.vpFixedKFs[r] = KeyFrameOf(fixedKeys[r]);
        if (!P.vpFixedKFs[r]) return hipdetail::Fail(who, "a row of the table without its key frame");
    }
    for (int e = 0; e < ne; e++) {
        const int kf = edges[e].kf;
        if (kf < 0 || kf >= nkf + nf || edges[e].idx < 0) return hipdetail::Fail(who, "an edge outside the lists");
        const BAEdge edge = {kf < nkf ? vpLocal[kf] : P.vpFixedKFs[kf - nkf], (size_t)edges[e].idx};
        P.vEdges[e] = edge;
    }
    P.vEdgeOff.assign(off.begin(), off.begin() + np + 1);
    for (int j = 0; j < np; j++) P.vpLocalMPs[j]->mnBALocalForKF = nStamp;    // ref: :2799
    for (int r = 0; r < nf; r++) P.vpFixedKFs[r]->mnBAFixedForKF = nStamp;    // ref: :2815
    std::swap(out, P);
    return true;
}

}  // namespace ORB_SLAM2
