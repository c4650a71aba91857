// LocalMap.cc -- host side of ORB_SLAM2::LocalMapSearch (include/orbhip/LocalMap.h): marshals MapPoint / Frame members into
// the orbhip_map_* / orbhip_search_local_points calls and writes the results back the way the reference's loops do
// (ref: src/Tracking.cc:2336-2364, src/Frame.cc:613-669, src/ORBmatcher.cc:45-129).
#include "LocalMap.h"

#include <cstdint>
#include <cstring>

#include "LocalMapDetail.h"
#include "hiperror.h"
#include "orbhip.h"

namespace ORB_SLAM2
{

namespace
{
int g_localmap_device = 0;
using localmapdetail::flags_of;
using localmapdetail::key_of;
}  // namespace

void LocalMapSearch::SetDevice(int device) { g_localmap_device = device; }

LocalMapSearch::LocalMapSearch(int maxPoints) : mpCtx(NULL)
{
    mpCtx = orbhip_create(g_localmap_device, 50, 1.2f, 1, 20, 7, 128, 128, 1);   // the smallest context: only its stream is used
    if (!mpCtx) {
        hipdetail::Fail("LocalMapSearch (device context)", orbhip_last_error(NULL));
        return;
    }
    if (orbhip_map_init(mpCtx, maxPoints) != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch (orbhip_map_init)", orbhip_last_error(mpCtx));
        orbhip_destroy(mpCtx);
        mpCtx = NULL;
        return;
    }
    orbhip_set_limit(mpCtx, 4);   // the frames being tracked: a handful at a time
}

LocalMapSearch::~LocalMapSearch()
{
    if (mpCtx) orbhip_destroy(mpCtx);
}

void LocalMapSearch::Put(MapPoint *pMP) { Put(std::vector<MapPoint *>(1, pMP)); }

void LocalMapSearch::Put(const std::vector<MapPoint *> &vpMPs)
{
    std::unique_lock<std::mutex> lock(mMutex);
    PutLocked(vpMPs);
}

bool LocalMapSearch::PutLocked(const std::vector<MapPoint *> &vpMPs)
{
    if (!mpCtx) return false;
    if (vpMPs.empty()) return true;
    const size_t n = vpMPs.size();
    std::vector<uint64_t> keys(n);
    std::vector<float> pos(3 * n), nrm(3 * n), mn(n), mx(n);
    std::vector<uint8_t> desc(32 * n), fl(n);
    for (size_t i = 0; i < n; i++) {
        MapPoint *p = vpMPs[i];
        keys[i] = key_of(p);
        const cv::Mat P = p->GetWorldPos(), N = p->GetNormal(), d = p->GetDescriptor();
        for (int k = 0; k < 3; k++) {
            pos[3 * i + k] = P.at<float>(k, 0);
            nrm[3 * i + k] = N.at<float>(k, 0);
        }
        // the raw mfMinDistance / mfMaxDistance: the accessors multiply by 0.8f / 1.2f (ref: src/MapPoint.cc:388-398), and
        // both are exact to undo only by reading the members -- protected in the reference, so LocalMapSearch is a friend
        // there
        mn[i] = p->mfMinDistance;
        mx[i] = p->mfMaxDistance;
        memcpy(&desc[32 * i], d.ptr(0), 32);
        fl[i] = flags_of(p);
    }
    if (orbhip_map_put(mpCtx, (int)n, keys.data(), pos.data(), nrm.data(), mn.data(), mx.data(), desc.data(), fl.data()) != ORBHIP_OK) {
        hipdetail::Fail("LocalMapSearch::Put", orbhip_last_error(mpCtx));
        return false;
    }
    for (size_t i = 0; i < n; i++) mPointOf[keys[i]] = vpMPs[i];
    return true;
}

MapPoint *LocalMapSearch::PointOf(uint64_t key) const
{
    const std::unordered_map<uint64_t, MapPoint *>::const_iterator it = mPointOf.find(key);
    return it == mPointOf.end() ? static_cast<MapPoint *>(NULL) : it->second;
}

bool LocalMapSearch::Known(MapPoint *pMP) const { return mPointOf.count(key_of(pMP)) != 0; }

bool LocalMapSearch::AllKnown(const std::vector<MapPoint *> &vpMPs) const
{
    for (size_t i = 0; i < vpMPs.size(); i++)
        if (vpMPs[i] && !vpMPs[i]->isBad() && !Known(vpMPs[i])) return false;
    return true;
}

void LocalMapSearch::PointsOf(const uint64_t *keys, int n, std::vector<MapPoint *> &out) const
{
    out.assign(n > 0 ? n : 0, static_cast<MapPoint *>(NULL));
    for (int k = 0; k < n; k++) out[k] = PointOf(keys[k]);
}

bool LocalMapSearch::UpdateFlagsLocked(MapPoint *const *points, size_t n, const char *who)
{
    if (n == 0) return true;
    uint64_t key1;   // one point (UpdateFlags, once per AddObservation) takes no allocation
    uint8_t fl1;
    std::vector<uint64_t> keys(n > 1 ? n : 0);
    std::vector<uint8_t> fls(keys.size());
    uint64_t *k = n > 1 ? keys.data() : &key1;
    uint8_t *f = n > 1 ? fls.data() : &fl1;
    for (size_t i = 0; i < n; i++) k[i] = key_of(points[i]), f[i] = flags_of(points[i]);
    if (orbhip_map_update_flags(mpCtx, (int)n, k, f) != ORBHIP_OK) return hipdetail::Fail(who, orbhip_last_error(mpCtx));
    return true;
}

void LocalMapSearch::AssignNormalDepth(MapPoint *pMP, const float *nrm, float minDistance, float maxDistance)
{
    cv::Mat n(3, 1, CV_32F);
    for (int c = 0; c < 3; c++) n.at<float>(c, 0) = nrm[c];
    pMP->mNormalVector = n;
    pMP->mfMinDistance = minDistance, pMP->mfMaxDistance = maxDistance;
}

void LocalMapSearch::UpdateFlags(MapPoint *pMP)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    UpdateFlagsLocked(&pMP, 1, "LocalMapSearch::UpdateFlags");
}

void LocalMapSearch::Erase(MapPoint *pMP)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    const uint64_t key = key_of(pMP);
    mPointOf.erase(key);
    if (orbhip_map_erase(mpCtx, 1, &key) != ORBHIP_OK) hipdetail::Fail("LocalMapSearch::Erase", orbhip_last_error(mpCtx));
}

void LocalMapSearch::Clear()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mpCtx) return;
    mPointOf.clear();
    if (orbhip_map_clear(mpCtx) != ORBHIP_OK || orbhip_set_drop(mpCtx, 0) != ORBHIP_OK)
        hipdetail::Fail("LocalMapSearch::Clear", orbhip_last_error(mpCtx));
}

int LocalMapSearch::SearchLocalPoints(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, float th, float viewingCosLimit,
                                      int *nToMatch)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (nToMatch) *nToMatch = 0;
    if (!mpCtx) return 0;
    const int n = F.N, nq = (int)vpLocalMapPoints.size();
    if (nq == 0) return 0;
    if (!localmapdetail::has_pyramid(F))
        return hipdetail::Fail("LocalMapSearch::SearchLocalPoints", "the frame has no scale pyramid (mnScaleLevels, mvScaleFactors)"), 0;

    uint64_t frameKey = 0;
    if (!localmapdetail::put_frame(mpCtx, F, &frameKey)) return hipdetail::Fail("LocalMapSearch::SearchLocalPoints (orbhip_set_put)", orbhip_last_error(mpCtx)), 0;
    orbhip_local_camera cam;
    localmapdetail::fill_camera(F, th, viewingCosLimit, &cam);

    std::vector<uint64_t> keys(nq);
    std::vector<uint8_t> skip(nq), occupied;
    for (int k = 0; k < nq; k++) {
        keys[k] = key_of(vpLocalMapPoints[k]);
        skip[k] = vpLocalMapPoints[k]->mnLastFrameSeen == F.mnId ? 1 : 0;     // ref: src/Tracking.cc:2342
    }
    localmapdetail::fill_occupied(F, occupied);
    std::vector<orbhip_local_point> pts(nq);
    std::vector<int32_t> match(n > 0 ? n : 1);
    int ntm = 0, found = 0;
    const int rc = orbhip_search_local_points(mpCtx, frameKey, (n > 0 && (int)F.mvuRight.size() == n) ? F.mvuRight.data() : NULL,
                                              occupied.data(), &cam, keys.data(), skip.data(), nq, 0.8f, pts.data(), &ntm,
                                              match.data(), &found);   // 0.8: the matcher Tracking constructs here
    if (rc != ORBHIP_OK) return hipdetail::Fail("LocalMapSearch::SearchLocalPoints", orbhip_last_error(mpCtx)), 0;
    localmapdetail::write_back(F, vpLocalMapPoints, skip, pts, match);
    if (nToMatch) *nToMatch = ntm;
    return found;
}

}  // namespace ORB_SLAM2
