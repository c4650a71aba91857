// LocalMapSim3.cc -- LocalMapSearch::SearchBySim3 (include/orbhip/LocalMap.h): ORBmatcher::SearchBySim3 of LoopClosing::ComputeSim3
// (ref: src/ORBmatcher.cc:1102-1326, src/LoopClosing.cc:375) as one orbhip_search_by_sim3 call on the resident store, the two key
// frames' rows and their feature sets.  The similarity between the cameras is composed here as
// ORBmatcher::SearchBySim3 composes it; the matches come back as feature indices and become MapPoint* from GetMapPointMatches().
// A pair the table cannot speak for goes the way that existed before: the call returns -1 and the caller runs
// ORBmatcher::SearchBySim3.  A file of its own: programs that link the other LocalMap*.cc files alone do not need the entry point.
#include "LocalMapDetail.h"
#include "../MatcherDetail.h"
#include "hiperror.h"

namespace ORB_SLAM2
{

using localmapdetail::fill_target;
using localmapdetail::has_pyramid;
using localmapdetail::key_of;

namespace
{
const int TH_HIGH = 100;   // ORBmatcher::TH_HIGH
}

int LocalMapSearch::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, const float &s12, const cv::Mat &R12,
                                 const cv::Mat &t12, const float th)
{
    std::unique_lock<std::mutex> lock(mMutex);
    if (!mbKeyFrames) return -1;
    KeyFrame *kf[2] = {pKF1, pKF2};
    std::vector<MapPoint *> points[2];
    for (int s = 0; s < 2; s++) {
        // can the table speak for the key frame?  It has a row, and every non-NULL, non-bad point is known to the store
        if (!HasRow(kf[s]) || !has_pyramid(kf[s])) return -1;   // (tests, does not put: the caller's way out is the host matcher)
        points[s] = kf[s]->GetMapPointMatches();
        if (points[s].empty() || (int)points[s].size() != kf[s]->mDescriptors.rows || !AllKnown(points[s])) return -1;
    }
    const int N1 = (int)points[0].size(), N2 = (int)points[1].size();
    if ((int)vpMatches12.size() != N1) return -1;

    orbhip_fuse_target sides[2];
    uint64_t rowKeys[2];
    for (int s = 0; s < 2; s++) {
        uint64_t setKey = 0;
        if (!EnsureFuseSet(kf[s], &setKey)) return hipdetail::Fail("LocalMapSearch::SearchBySim3 (key frame set)", orbhip_last_error(mpCtx)), -1;
        fill_target(kf[s], setKey, th, &sides[s]);
        rowKeys[s] = key_of(kf[s]);
    }

    // the similarity between the cameras, both ways (ref: :1119-1121)
    cv::Mat sR12, sR21;
    hipdetail::scale3(R12, (double)s12, false, sR12);                     // s12*R12
    hipdetail::scale3(R12, 1.0 / s12, true, sR21);                        // (1.0/s12)*R12.t()
    float t12v[3], t21[3], r12[9], r21[9];
    for (int r = 0; r < 3; r++) {
        t12v[r] = t12.at<float>(r, 0);
        for (int c = 0; c < 3; c++) r12[3 * r + c] = sR12.at<float>(r, c), r21[3 * r + c] = sR21.at<float>(r, c);
    }
    hipdetail::affine3(sR21, t12v, NULL, t21, false, -1.0);               // t21 = -sR21*t12

    // what the caller has matched already stays out of both searches (ref: :1129-1142)
    std::vector<uint8_t> taken1(N1, 0), taken2(N2, 0);
    for (int i = 0; i < N1; i++) {
        MapPoint *pMP = vpMatches12[i];
        if (!pMP) continue;
        taken1[i] = 1;
        const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
        if (idx2 >= 0 && idx2 < N2) taken2[idx2] = 1;
    }

    std::vector<int32_t> match12(N1);
    int nFound = 0;
    int32_t nActive[2] = {0, 0};
    if (orbhip_search_by_sim3(mpCtx, sides, rowKeys, r21, t21, r12, t12v, th, TH_HIGH, taken1.data(), taken2.data(), match12.data(), &nFound,
                              nActive, NULL, NULL, NULL, NULL, NULL, NULL) != ORBHIP_OK)
        return hipdetail::Fail("LocalMapSearch::SearchBySim3", orbhip_last_error(mpCtx)), -1;
    for (int i1 = 0; i1 < N1; i1++)
        if (match12[i1] >= 0 && match12[i1] < N2) vpMatches12[i1] = points[1][match12[i1]];   // ref: :1319
    return nFound;
}

}  // namespace ORB_SLAM2
