// TriangulationSearch.cc -- host side of ORB_SLAM2::TriangulationSearch (include/orbhip/TriangulationSearch.h): makes the
// K + 1 key frames resident, packs what changes from call to call, makes the one orbhip_search_for_triangulation_sets call and
// turns the match rows into pair lists.
#include "TriangulationSearch.h"

#include <algorithm>
#include <cstdint>

#include "../MatcherDetail.h"
#include "hiperror.h"
#include "orbhip.h"

namespace ORB_SLAM2
{

namespace
{
int g_tri_device = 0;
const int kMaxSets = 96;                      // the most orbhip_set_limit grants
}  // namespace

void TriangulationSearch::SetDevice(int device) { g_tri_device = device; }

TriangulationSearch::TriangulationSearch() : mpCtx(NULL), mnSetLimit(kMaxSets)
{
    mpCtx = orbhip_create(g_tri_device, 50, 1.2f, 1, 20, 7, 128, 128, 1);   // the smallest context: its stream and its set table are used
    if (!mpCtx) hipdetail::Fail("TriangulationSearch (device context)", orbhip_last_error(NULL));
}

TriangulationSearch::~TriangulationSearch()
{
    if (mpCtx) orbhip_destroy(mpCtx);
}

void TriangulationSearch::SetResidentSetLimit(int n)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (mpCtx) mnSetLimit = orbhip_set_limit(mpCtx, n);
}

void TriangulationSearch::DropResidentSets()
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (mpCtx) orbhip_set_drop(mpCtx, 0);
}

int TriangulationSearch::SearchForTriangulation(KeyFrame *pKF1, const std::vector<KeyFrame*> &vpKF2, const std::vector<cv::Mat> &vF12,
                                                std::vector<std::vector<std::pair<size_t,size_t> > > &vvMatchedPairs,
                                                bool bOnlyStereo, bool bCheckOrientation)
{
    const char *who = "TriangulationSearch::SearchForTriangulation";
    std::unique_lock<std::mutex> lock(mMutex);
    vvMatchedPairs.assign(vpKF2.size(), std::vector<std::pair<size_t,size_t> >());
    if (!mpCtx) return hipdetail::Fail(who, "no device context"), 0;
    if (!pKF1 || vF12.size() != vpKF2.size()) return hipdetail::Fail(who, "vF12 must hold one matrix per key frame of vpKF2"), 0;
    const int n1 = pKF1->N;
    if (n1 == 0) return 0;
    // a key frame without features has no set and no matches (the reference returns 0 for it)
    std::vector<int> act;
    for (size_t k = 0; k < vpKF2.size(); k++) {
        if (!vpKF2[k]) return hipdetail::Fail(who, "null key frame in vpKF2"), 0;
        if (vF12[k].rows != 3 || vF12[k].cols != 3 || vF12[k].type() != CV_32F) return hipdetail::Fail(who, "F12 must be 3x3 CV_32F"), 0;
        if (vpKF2[k]->N > 0) act.push_back((int)k);
    }
    if (act.empty()) return 0;
    const KeyFrame *pLevels = vpKF2[act[0]];
    for (size_t a = 1; a < act.size(); a++)
        if (vpKF2[act[a]]->mvScaleFactors != pLevels->mvScaleFactors || vpKF2[act[a]]->mvLevelSigma2 != pLevels->mvLevelSigma2)
            return hipdetail::Fail(who, "the neighbours of one call must share mvScaleFactors and mvLevelSigma2"), 0;
    if (pLevels->mvLevelSigma2.size() != pLevels->mvScaleFactors.size())
        return hipdetail::Fail(who, "mvScaleFactors and mvLevelSigma2 differ in length"), 0;

    std::vector<uint8_t> skip1(n1);
    for (int i = 0; i < n1; i++) skip1[i] = pKF1->GetMapPoint(i) ? 1 : 0;     // ref: src/ORBmatcher.cc:702-705
    const float *ur1 = (int)pKF1->mvuRight.size() == n1 ? pKF1->mvuRight.data() : NULL;

    int total = 0;
    // (all the neighbours in one call; more than the table can hold beside key frame 1 go in further calls)
    for (size_t first = 0; first < act.size(); first += kMaxSets - 1) {
        const int K = (int)std::min(act.size() - first, (size_t)(kMaxSets - 1));
        if (K + 1 > mnSetLimit) mnSetLimit = orbhip_set_limit(mpCtx, K + 1);
        // key frame 1 last: of K + 1 sets it is then the most recently used one
        std::vector<orbhip_tri_neighbour> nb(K);
        std::vector<uint8_t> skip2;
        std::vector<float> ur2;
        bool anyStereo2 = false;
        for (int j = 0; j < K; j++) {
            KeyFrame *pKF2 = vpKF2[act[first + j]];
            if (!hipdetail::ensure_set(mpCtx, (uint64_t)pKF2->mnId + 1, *pKF2, pKF2->mvKeysUn, pKF2->mnMinX, pKF2->mnMinY,
                                       pKF2->mfGridElementWidthInv, pKF2->mfGridElementHeightInv, NULL))
                return hipdetail::Fail(who, orbhip_last_error(mpCtx)), 0;
            const int n2 = pKF2->N;
            nb[j].key2 = (uint64_t)pKF2->mnId + 1;
            const cv::Mat &F12 = vF12[act[first + j]];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) nb[j].F12[3 * r + c] = F12.at<float>(r, c);
            hipdetail::epipole_in_second(pKF1, pKF2, nb[j].ex, nb[j].ey);
            for (int i = 0; i < n2; i++) skip2.push_back(pKF2->GetMapPoint(i) ? 1 : 0);     // ref: :727-731
            const bool stereo2 = (int)pKF2->mvuRight.size() == n2;
            anyStereo2 |= stereo2;
            for (int i = 0; i < n2; i++) ur2.push_back(stereo2 ? pKF2->mvuRight[i] : -1.0f);   // (negative: a monocular feature)
        }
        if (!hipdetail::ensure_set(mpCtx, (uint64_t)pKF1->mnId + 1, *pKF1, pKF1->mvKeysUn, pKF1->mnMinX, pKF1->mnMinY,
                                   pKF1->mfGridElementWidthInv, pKF1->mfGridElementHeightInv, NULL))
            return hipdetail::Fail(who, orbhip_last_error(mpCtx)), 0;
        std::vector<int32_t> m12((size_t)K * n1), nm(K);
        const int rc = orbhip_search_for_triangulation_sets(
            mpCtx, (uint64_t)pKF1->mnId + 1, skip1.data(), ur1, nb.data(), K, skip2.data(), anyStereo2 ? ur2.data() : NULL,
            pLevels->mvScaleFactors.data(), pLevels->mvLevelSigma2.data(), (int)pLevels->mvScaleFactors.size(), bOnlyStereo ? 1 : 0,
            bCheckOrientation ? 1 : 0, m12.data(), nm.data());
        if (rc != ORBHIP_OK) {
            vvMatchedPairs.assign(vpKF2.size(), std::vector<std::pair<size_t,size_t> >());
            return hipdetail::Fail(who, orbhip_last_error(mpCtx)), 0;
        }
        for (int j = 0; j < K; j++) {
            std::vector<std::pair<size_t,size_t> > &pairs = vvMatchedPairs[act[first + j]];
            pairs.reserve(nm[j]);
            for (int i = 0; i < n1; i++)
                if (m12[(size_t)j * n1 + i] >= 0) pairs.push_back(std::pair<size_t,size_t>(i, m12[(size_t)j * n1 + i]));
            total += nm[j];
        }
    }
    return total;
}

}  // namespace ORB_SLAM2
