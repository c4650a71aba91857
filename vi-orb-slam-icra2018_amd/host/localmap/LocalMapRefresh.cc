// LocalMapRefresh.cc -- LocalMapSearch::RefreshPoints (include/orbhip/LocalMap.h): MapPoint::ComputeDistinctiveDescriptors and
// MapPoint::UpdateNormalAndDepth for a batch of points as one orbhip_map_refresh call on the resident store and feature sets
// (ref: src/MapPoint.cc:257-322, :345-386, the loops of src/LocalMapping.cc:2036-2046 and :2577-2590), the
// results assigned to the caller's objects.  Points the call cannot serve go the way that existed before it: the per-point methods
// on the host, then one Put.  A file of its own: programs that link the other LocalMap*.cc files alone do not need the entry point.
#include <algorithm>
#include <cstring>
#include <map>
#include <set>

#include "LocalMapDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::key_of;

int LocalMapSearch::SetLimit(int maxSets)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return 0;
    mbFuseSets = true;   // (EnsureFuseSet leaves the limit alone from now on)
    return mnSetLimit = orbhip_set_limit(mpCtx, maxSets);
}

int LocalMapSearch::RefreshPoints(const std::vector<MapPoint *> &vpMPs, bool bDescriptors, bool bNormals)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx || (!bDescriptors && !bNormals)) return 0;
    typedef localmapdetail::ObservationList List;   // a point's observations in ascending KeyFrame::mnId
    std::vector<MapPoint *> pts;
    std::vector<List> lists;
    std::set<MapPoint *> seen;
    std::map<long unsigned int, KeyFrame *> observers;          // every observer of the call, by mnId
    for (size_t i = 0; i < vpMPs.size(); i++) {
        MapPoint *p = vpMPs[i];
        if (!p || p->isBad() || !seen.insert(p).second) continue;
        const List l = localmapdetail::observations_by_mnid(p);
        if (l.empty()) continue;                                 // (both methods return at once)
        for (size_t j = 0; j < l.size(); j++) observers[l[j].first->mnId] = l[j].first;
        pts.push_back(p);
        lists.push_back(l);
    }
    if (pts.empty()) return 0;

    // the observers whose features are (or become) resident sets: in ascending mnId, up to the set limit in force
    std::map<KeyFrame *, int> kfIndex;
    std::vector<orbhip_refresh_kf> kfs;
    KeyFrame *pyramid = NULL;
    for (std::map<long unsigned int, KeyFrame *>::const_iterator it = observers.begin(); it != observers.end(); ++it) {
        KeyFrame *kf = it->second;
        uint64_t setKey = 0;
        if (mbFuseSets && (int)kfs.size() >= mnSetLimit) break;
        if (!localmapdetail::has_pyramid(kf) || !EnsureFuseSet(kf, &setKey)) continue;   // (the object's first EnsureFuseSet raises the limit)
        if (!pyramid) pyramid = kf;
        orbhip_refresh_kf r;
        memset(&r, 0, sizeof r);
        r.set_key = setKey;
        const cv::Mat O = kf->GetCameraCenter();
        for (int c = 0; c < 3; c++) r.Ow[c] = O.at<float>(c, 0);
        r.flags = kf->isBad() ? ORBHIP_KF_BAD : 0;
        kfIndex[kf] = (int)kfs.size();
        kfs.push_back(r);
    }

    std::vector<MapPoint *> dev, host;
    std::vector<uint64_t> keys;
    std::vector<int32_t> off(1, 0), obsKf, obsIdx, refPos;
    for (size_t i = 0; i < pts.size(); i++) {
        MapPoint *p = pts[i];
        const List &l = lists[i];
        bool ok = Known(p);
        int ref = 0;
        for (size_t j = 0; j < l.size() && ok; j++) {
            ok = kfIndex.count(l[j].first) != 0 && (int)l[j].second < l[j].first->N;
            if (l[j].first == p->mpRefKF) ref = (int)j;
        }
        if (ok && bNormals) ok = p->mpRefKF && l[ref].first == p->mpRefKF;
        if (!ok) {
            host.push_back(p);
            continue;
        }
        dev.push_back(p);
        keys.push_back(key_of(p));
        for (size_t j = 0; j < l.size(); j++) obsKf.push_back(kfIndex[l[j].first]), obsIdx.push_back((int32_t)l[j].second);
        off.push_back((int32_t)obsKf.size());
        refPos.push_back(ref);
    }

    int touched = 0;
    if (!dev.empty()) {
        const int P = (int)dev.size();
        orbhip_refresh_params prm;
        localmapdetail::fill_refresh_params(pyramid, &prm);
        prm.what = (bDescriptors ? ORBHIP_REFRESH_DESC : 0) | (bNormals ? ORBHIP_REFRESH_NORMAL : 0);
        std::vector<uint8_t> status(P), desc((size_t)P * 32);
        std::vector<float> nrm((size_t)P * 3), mn(P), mx(P);
        if (orbhip_map_refresh(mpCtx, &prm, (int)kfs.size(), kfs.data(), P, keys.data(), off.data(), obsKf.data(), obsIdx.data(),
                               refPos.data(), status.data(), NULL, desc.data(), nrm.data(), mn.data(), mx.data()) != ORBHIP_OK) {
            hipdetail::Fail("LocalMapSearch::RefreshPoints", orbhip_last_error(mpCtx));
            host.insert(host.end(), dev.begin(), dev.end());     // the map stays right: these go the host way as well
        } else {
            for (int i = 0; i < P; i++) {
                MapPoint *p = dev[i];
                if (status[i] & ORBHIP_REFRESH_DESC) {
                    cv::Mat d(1, 32, CV_8U);
                    memcpy(d.ptr(0), &desc[(size_t)i * 32], 32);
                    p->mDescriptor = d;
                }
                if (status[i] & ORBHIP_REFRESH_NORMAL) AssignNormalDepth(p, &nrm[(size_t)i * 3], mn[i], mx[i]);
            }
            touched += P;
            RefreshCounts().device += P;
        }
    }
    if (!host.empty()) {
        for (size_t i = 0; i < host.size(); i++) {
            if (bDescriptors) host[i]->ComputeDistinctiveDescriptors();
            if (bNormals) host[i]->UpdateNormalAndDepth();
        }
        if (PutLocked(host)) touched += (int)host.size();
        RefreshCounts().host += (long)host.size();
    }
    return touched;
}

}  // namespace ORB_SLAM2
