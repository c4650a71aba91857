// slamlite.h -- the members of ORB_SLAM2::Frame / KeyFrame / MapPoint and DBoW2::FeatureVector
// that ORBmatcher::SearchByBoW reads (ref: src/ORBmatcher.cc:159-288, 522-655) and that
// Frame::ComputeStereoMatches reads and writes (ref: src/Frame.cc:810-984), for builds
// outside the reference tree.  Inside the reference tree define ORBHIP_WITH_REFERENCE_HEADERS and
// the real "Frame.h" / "KeyFrame.h" / "MapPoint.h" are included instead.
#ifndef ORBHIP_SLAMLITE_H
#define ORBHIP_SLAMLITE_H

#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "cvlite.h"

namespace DBoW2
{
typedef unsigned int NodeId;
typedef unsigned int WordId;
typedef double WordValue;
// ref: Thirdparty/DBoW2/DBoW2/BowVector.h -- word id -> value
class BowVector : public std::map<WordId, WordValue>
{
};
// ref: Thirdparty/DBoW2/DBoW2/FeatureVector.h -- node id -> indices of the features under it
class FeatureVector : public std::map<NodeId, std::vector<unsigned int> >
{
public:
    void addFeature(NodeId id, unsigned int i_feature) { (*this)[id].push_back(i_feature); }
};
}  // namespace DBoW2

namespace ORB_SLAM2
{

class Frame;
class KeyFrame;

class MapPoint
{
public:
    MapPoint() : mnId(NextId()++), mTrackProjX(0), mTrackProjY(0), mTrackProjXR(0), mbTrackInView(false), mnTrackScaleLevel(0),
                 mTrackViewCos(0), mnLastFrameSeen(0), nObs(0), mfMinDistance(0), mfMaxDistance(0), mpReplaced(0), mbBad(false) {}
    bool isBad() { return mbBad; }          // ref: include/MapPoint.h
    void SetBadFlag() { mbBad = true; }
    int Observations() { return nObs; }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }   // ref: src/MapPoint.cc:75-80
    float GetMinDistanceInvariance() { return 0.8f*mfMinDistance; }   // ref: src/MapPoint.cc:388-398
    float GetMaxDistanceInvariance() { return 1.2f*mfMaxDistance; }
    int PredictScale(const float &currentDist, Frame *pF);           // ref: src/MapPoint.cc:417-432 (body below Frame)
    int PredictScale(const float &currentDist, KeyFrame *pKF);       // ref: src/MapPoint.cc:400-415 (body below KeyFrame)

    // the map operations ORBmatcher::Fuse / SearchBySim3 call (ref: src/MapPoint.cc:113-124, 192-230, 366-386; bodies
    // below KeyFrame).  Replace moves the observations and marks this point bad; the reference's Replace also merges the
    // found / visible counters, recomputes the survivor's descriptor and erases the point from the Map, which have no
    // twin here (none of it is read again inside the matcher).
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    bool IsInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    void AddObservation(KeyFrame *pKF, size_t idx);
    // ref: src/MapPoint.cc:126-157 (body below KeyFrame): nObs goes down by 1, or by 2 for a stereo observation; mpRefKF, when it
    // was pKF, becomes the remaining observer of lowest mnId (the reference takes the lowest heap address); at nObs <= 2 the
    // reference's SetBadFlag follows: the flag, and EraseMapPointMatch in every remaining observer (the Map edit is not modelled)
    void EraseObservation(KeyFrame *pKF);
    void Replace(MapPoint *pMP);
    MapPoint *GetReplaced() { return mpReplaced; }
    void SetDescriptor(const cv::Mat &d) { mDescriptor = d.clone(); }   // mDescriptor is protected in the reference
    // ref: src/MapPoint.cc:283-349 (body below KeyFrame): the observed descriptor with the least median distance to the others.
    // The reference walks its observation map by heap address; here the observations are taken in ascending KeyFrame::mnId
    // order, so that equal medians resolve the same way in every process.  The reference's Replace ends in this call
    // (src/MapPoint.cc:227); here it does so only while RecomputeOnReplace() is set, which the programs that test
    // LocalMapSearch::FuseInTargets do (a survivor's descriptor then changes between two targets, as in the reference).
    void ComputeDistinctiveDescriptors();
    // ref: src/MapPoint.cc:345-386 (body below KeyFrame): mNormalVector, mfMinDistance, mfMaxDistance from the observers' camera
    // centres and mpRefKF's feature, written with the explicit operations docs/parity.md fixes ("UpdateNormalAndDepth"); the
    // observations are walked in ascending KeyFrame::mnId.  Nothing happens while mpRefKF is NULL.
    void UpdateNormalAndDepth();
    KeyFrame *mpRefKF = 0;                   // ref: include/MapPoint.h (protected there)
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    // Variables used by loop closing (ref: include/MapPoint.h:113-117): the stamps LoopClosing::CorrectLoop leaves on a point it
    // moved, and what RunGlobalBundleAdjustment reads (LocalMapSearch::CorrectLoopPoints / ApplyGlobalBA)
    long unsigned int mnCorrectedByKF = 0;
    long unsigned int mnCorrectedReference = 0;
    cv::Mat mPosGBA;                         // 3 x 1 CV_32F
    long unsigned int mnBAGlobalForKF = 0;
    // Variable used by local mapping (ref: include/MapPoint.h:110): the stamp of Optimizer::LocalBundleAdjustment's point walk,
    // left by LocalMapSearch::BuildLocalBA / BuildBAProblem
    long unsigned int mnBALocalForKF = 0;
    static bool &RecomputeOnReplace() { static bool b = false; return b; }

    // ref: include/MapPoint.h "long unsigned int mnId; static long unsigned int nNextId;": mnId + 1 is the key under which
    // LocalMapSearch keeps the point resident on the device
    long unsigned int mnId;
    static long unsigned int &NextId() { static long unsigned int n = 0; return n; }

    // Variables used by the tracking (ref: include/MapPoint.h:102-107), read by SearchByProjection
    float mTrackProjX;
    float mTrackProjY;
    float mTrackProjXR;
    bool mbTrackInView;
    int mnTrackScaleLevel;
    float mTrackViewCos;
    long unsigned int mnLastFrameSeen;       // ref: include/MapPoint.h (set by Tracking::SearchLocalPoints' first loop)
    long unsigned int mnTrackReferenceForFrame = 0;   // ref: include/MapPoint.h (set by Tracking::UpdateLocalPoints)

    // protected in the reference; the test programs fill them directly
    int nObs;
    cv::Mat mDescriptor;                     // 1 x 32 CV_8U
    cv::Mat mWorldPos;                       // 3 x 1 CV_32F
    float mfMinDistance, mfMaxDistance;      // scale invariance distances
    cv::Mat mNormalVector;                   // 3 x 1 CV_32F, mean viewing direction
    std::map<KeyFrame *, size_t> mObservations;
    MapPoint *mpReplaced;
protected:
    bool mbBad;
};

class ORBextractor;
class ORBVocabulary;

#define FRAME_GRID_ROWS 48                   // ref: include/Frame.h:41-42
#define FRAME_GRID_COLS 64

class Frame
{
public:
    Frame() : mnId(NextId()++), N(0), mpORBvocabulary(0), mnScaleLevels(0), mfScaleFactor(0), mfLogScaleFactor(0),
              mpORBextractorLeft(0), mpORBextractorRight(0), mbf(0), mb(0) {}
    // ref: include/Frame.h "static long unsigned int nNextId; long unsigned int mnId;" (src/Frame.cc: mnId=nNextId++), the
    // key under which the drop-in matcher keeps a frame's descriptors resident on the device
    long unsigned int mnId;
    static long unsigned int &NextId() { static long unsigned int n = 0; return n; }
    int N;                                   // ref: include/Frame.h
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    std::vector<MapPoint *> mvpMapPoints;
    // ref: include/Frame.h (mpORBvocabulary, mBowVec) and src/Frame.cc:739-746; body in host/FrameGrid.cc: the by-products of
    // the extractor's frame build when it has them, ORBVocabulary::transform otherwise
    ORBVocabulary *mpORBvocabulary;
    DBoW2::BowVector mBowVec;
    void ComputeBoW();

    // grid and guided-search members (ref: include/Frame.h:187-262) and the methods of src/Frame.cc:574-589,
    // :671-724; bodies in vi-orb-slam-icra2018_amd/host/FrameGrid.cc (device grid through liborbhip)
    static float fx, fy, cx, cy;
    static float mnMinX, mnMaxX, mnMinY, mnMaxY;
    static float mfGridElementWidthInv, mfGridElementHeightInv;
    std::vector<bool> mvbOutlier;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    cv::Mat mTcw;                            // 4 x 4 CV_32F
    std::vector<float> mvScaleFactors, mvLevelSigma2;   // (mvLevelSigma2: read by PnPsolver::PnPsolver, ref: src/PnPsolver.cc:90)
    int mnScaleLevels;                       // ref: src/Frame.cc:61-63 (mfLogScaleFactor = log(mfScaleFactor), float)
    float mfScaleFactor, mfLogScaleFactor;
    cv::Mat mK;                              // 3 x 3 CV_32F
    cv::Mat mDistCoef;                       // 4 x 1 (or 5 / 8) CV_32F
    void UndistortKeyPoints();               // ref: src/Frame.cc:748-778
    void ComputeImageBounds(const cv::Mat &imLeft);   // ref: :780-808
    void AssignFeaturesToGrid();
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel = -1,
                                          const int maxLevel = -1) const;

    // stereo members (ref: include/Frame.h:124-176) and the method of src/Frame.cc:810-984.  The body in
    // vi-orb-slam-icra2018_amd/host/FrameStereo.cc runs on the pyramids the two extractors hold on the device.
    ORBextractor *mpORBextractorLeft, *mpORBextractorRight;
    std::vector<cv::KeyPoint> mvKeysRight;
    cv::Mat mDescriptorsRight;
    std::vector<float> mvuRight, mvDepth;
    float mbf, mb;
    void ComputeStereoMatches();
    // RGB-D (ref: include/Frame.h, src/Frame.cc:987-1008, called by the RGB-D constructor at :489); body in vi-orb-slam-icra2018_amd/host/rgbd/FrameRGBD.cc.  imDepth: the
    // CV_32F map Tracking::GrabImageRGBD converted (ref: src/Tracking.cc:924-925).  The overload takes the map as the sensor
    // delivers it, CV_16U or CV_32F, and Tracking's mDepthMapFactor: the convertTo goes away, only the pixels under the keypoints
    // are converted, with the same result.
    void ComputeStereoFromRGBD(const cv::Mat &imDepth);
    void ComputeStereoFromRGBD(const cv::Mat &imDepthRaw, float depthMapFactor);
};

inline int MapPoint::PredictScale(const float &currentDist, Frame *pF)
{
    const float ratio = mfMaxDistance/currentDist;
    int nScale = std::ceil(std::log(ratio)/pF->mfLogScaleFactor);
    if(nScale<0)
        nScale = 0;
    else if(nScale>=pF->mnScaleLevels)
        nScale = pF->mnScaleLevels-1;
    return nScale;
}

class KeyFrame
{
public:
    KeyFrame() : mnId(NextId()++), mbBad(false), N(0), fx(0), fy(0), cx(0), cy(0), mbf(0), mnScaleLevels(0), mfScaleFactor(0), mfLogScaleFactor(0),
                 mnGridCols(FRAME_GRID_COLS), mnGridRows(FRAME_GRID_ROWS),
                 mfGridElementWidthInv(0), mfGridElementHeightInv(0), mnMinX(0), mnMinY(0), mnMaxX(0), mnMaxY(0) {}
    long unsigned int mnId;                       // ref: include/KeyFrame.h (src/KeyFrame.cc:46: mnId=nNextId++)
    static long unsigned int &NextId() { static long unsigned int n = 0; return n; }
    bool isBad() { return mbBad; }                // ref: src/KeyFrame.cc (read by MapPoint::ComputeDistinctiveDescriptors)
    bool mbBad;
    // The observation half of KeyFrame::SetBadFlag (ref: src/KeyFrame.cc:952-1040): EraseObservation on every point, then mbBad;
    // mvpMapPoints stays as it is, as there; a key frame that is bad already returns at once, as there.  The edits of the covisibility graph, the spanning tree, the Map and the key-frame
    // database, and the mbNotErase / mbToBeErased hand-over with LoopClosing, are not modelled.  Read by LocalMapping::KeyFrameCulling
    // (ref: src/LocalMapping.cc:2692-2756): mvDepth (negative for monocular points) and mThDepth.
    void SetBadFlag()
    {
        if (mbBad || mnId == 0) return;
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mbBad = true;
    }
    std::vector<float> mvDepth;
    float mThDepth = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;   // ref: include/KeyFrame.h (const members there)
    cv::Mat mDescriptors;
    DBoW2::FeatureVector mFeatVec;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<MapPoint *> mvpMapPoints;

    // read by ORBmatcher::SearchForTriangulation (ref: src/ORBmatcher.cc:657-827)
    int N;
    float fx, fy, cx, cy;
    std::vector<float> mvuRight;                  // negative value for monocular points
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    // read / written by ORBmatcher::Fuse, SearchBySim3 and SearchByProjection(KeyFrame*, Scw, ...) (ref: src/ORBmatcher.cc:
    // 290-403, 825-1326; src/KeyFrame.cc:643-681)
    float mbf;
    int mnScaleLevels;
    float mfScaleFactor, mfLogScaleFactor;
    std::vector<float> mvInvLevelSigma2;
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(NULL); }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    std::set<MapPoint *> GetMapPoints()
    {
        std::set<MapPoint *> s;
        for (size_t i = 0, iend = mvpMapPoints.size(); i < iend; i++)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
        return s;
    }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }     // ref: src/KeyFrame.cc
    cv::Mat GetTranslation()
    {
        cv::Mat t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) t.at<float>(r, 0) = Tcw.at<float>(r, 3);
        return t;
    }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    // ref: src/KeyFrame.cc:95-118, :120-130.  Ow = -Rcw.t()*tcw is one gemm with alpha = -1: products summed in double, one
    // rounding (as host/MatcherDetail.h decompose_sim3 writes it); Twc = [Rcw.t() | Ow]
    void SetPose(const cv::Mat &Tcw_)
    {
        Tcw = Tcw_.clone();
        cv::Mat O(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)Tcw.at<float>(k, r) * (double)Tcw.at<float>(k, 3);
            O.at<float>(r, 0) = (float)(-1.0 * s + 0.0);
        }
        Ow = O;
    }
    cv::Mat GetPose() { return Tcw.clone(); }
    cv::Mat GetPoseInverse()
    {
        cv::Mat Twc = cv::Mat::zeros(4, 4, CV_32F);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Twc.at<float>(r, c) = Tcw.at<float>(c, r);
            Twc.at<float>(r, 3) = Ow.at<float>(r, 0);
        }
        Twc.at<float>(3, 3) = 1.f;
        return Twc;
    }
    // Variables used by loop closing (ref: include/KeyFrame.h:188-191): the pose before a global bundle adjustment and the stamp
    // of the adjustment that moved the key frame, read by LocalMapSearch::ApplyGlobalBA
    cv::Mat mTcwGBA;
    cv::Mat mTcwBefGBA;
    long unsigned int mnBAGlobalForKF = 0;
    // Variables used by the local mapping (ref: include/KeyFrame.h:184-185): the stamps Optimizer::LocalBundleAdjustment leaves on
    // its local and its fixed key frames (LocalMapSearch::BuildLocalBA / BuildBAProblem)
    long unsigned int mnBALocalForKF = 0;
    long unsigned int mnBAFixedForKF = 0;
    cv::Mat Tcw;                                  // 4 x 4 CV_32F (protected in the reference; the test programs fill it)
    cv::Mat Ow;                                   // 3 x 1 CV_32F

    // grid twin of the frame (ref: include/KeyFrame.h:226-229, 306; the constructor copies F.mGrid, src/KeyFrame.cc:55-89)
    // and KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:1138-1177: no level filter); body in host/ORBmatcher.cc
    int mnGridCols, mnGridRows;
    float mfGridElementWidthInv, mfGridElementHeightInv;
    float mnMinX, mnMinY, mnMaxX, mnMaxY;
    std::vector<std::vector<std::vector<size_t> > > mGrid;
    void CopyGridFrom(const Frame &F);            // the grid part of KeyFrame::KeyFrame(Frame &F, ...)
    std::vector<size_t> GetFeaturesInArea(const float &x, const float &y, const float &r) const;
    bool IsInImage(const float &x, const float &y) const { return (x>=mnMinX && x<mnMaxX && y>=mnMinY && y<mnMaxY); }

    // read and written by KeyFrameDatabase (ref: include/KeyFrame.h:240-245, src/KeyFrameDatabase.cc); initialised to 0 here
    // (the reference leaves mRelocScore uninitialised, src/KeyFrame.cc:58)
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    // the covisibility graph as KeyFrameDatabase reads it (ref: src/KeyFrame.cc GetConnectedKeyFrames /
    // GetBestCovisibilityKeyFrames over mvpOrderedConnectedKeyFrames): key frames by decreasing weight, filled by the caller
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> GetConnectedKeyFrames()
    {
        return std::set<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end());
    }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    // read and written by Tracking::UpdateLocalKeyFrames (ref: include/KeyFrame.h, src/Tracking.cc:2445-2527): the stamp that
    // keeps a key frame from entering the local map twice, and the spanning tree (filled by the caller)
    long unsigned int mnTrackReferenceForFrame = 0;
    std::set<KeyFrame *> mspChildrens;
    KeyFrame *mpParent = 0;
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    KeyFrame *GetParent() { return mpParent; }

    // the covisibility graph as KeyFrame::UpdateConnections builds it (ref: src/KeyFrame.cc:528-562, :731-843; bodies below
    // MapPoint's).  Where the reference orders by KeyFrame* (the walk of map<KeyFrame*, int>, the second member of the sorted
    // pairs) the order here is that of mnId, so that equal weights resolve the same way in every process (docs/parity.md):
    // mvpOrderedConnectedKeyFrames comes in descending weight, ties in descending mnId, and when no link reaches the threshold
    // the first maximum in ascending mnId is taken.  A caller may still fill mvpOrderedConnectedKeyFrames by hand instead.
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    void AddChild(KeyFrame *pKF) { mspChildrens.insert(pKF); }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame *> GetCovisiblesByWeight(const int &w);
    int GetWeight(KeyFrame *pKF) { return mConnectedKeyFrameWeights.count(pKF) ? mConnectedKeyFrameWeights[pKF] : 0; }
    void AddConnection(KeyFrame *pKF, const int &weight);
    void UpdateBestCovisibles();       // lists EVERY entry of mConnectedKeyFrameWeights, the ones below the threshold included
    void UpdateConnections();
    // (weight, key frame) pairs -> the two ordered lists: sort() ascending by (weight, mnId), then read from the back
    static void OrderCovisibles(std::vector<std::pair<int, KeyFrame *> > &vPairs, std::vector<KeyFrame *> &vpKFs, std::vector<int> &vWs);
};

inline int MapPoint::PredictScale(const float &currentDist, KeyFrame *pKF)
{
    const float ratio = mfMaxDistance/currentDist;
    int nScale = std::ceil(std::log(ratio)/pKF->mfLogScaleFactor);
    if(nScale<0)
        nScale = 0;
    else if(nScale>=pKF->mnScaleLevels)
        nScale = pKF->mnScaleLevels-1;
    return nScale;
}

inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx)
{
    if(mObservations.count(pKF))
        return;
    mObservations[pKF]=idx;
    if(idx<pKF->mvuRight.size() && pKF->mvuRight[idx]>=0)
        nObs+=2;
    else
        nObs++;
}

inline void MapPoint::EraseObservation(KeyFrame *pKF)
{
    bool bBad = false;
    if(mObservations.count(pKF))
    {
        const size_t idx = mObservations[pKF];
        if(idx<pKF->mvuRight.size() && pKF->mvuRight[idx]>=0)
            nObs-=2;
        else
            nObs--;
        mObservations.erase(pKF);
        if(mpRefKF==pKF)
        {
            mpRefKF = NULL;
            for(std::map<KeyFrame *, size_t>::iterator mit=mObservations.begin(), mend=mObservations.end(); mit!=mend; mit++)
                if(!mpRefKF || mit->first->mnId<mpRefKF->mnId)
                    mpRefKF = mit->first;
        }
        if(nObs<=2)
            bBad = true;
    }
    if(bBad)
    {
        const std::map<KeyFrame *, size_t> obs = mObservations;   // SetBadFlag of the reference (src/MapPoint.cc:165-183)
        mObservations.clear();
        mbBad = true;
        for(std::map<KeyFrame *, size_t>::const_iterator mit=obs.begin(), mend=obs.end(); mit!=mend; mit++)
            mit->first->EraseMapPointMatch(mit->second);
    }
}

inline void MapPoint::Replace(MapPoint *pMP)
{
    if(pMP==this)
        return;
    std::map<KeyFrame *, size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    mpReplaced = pMP;
    for(std::map<KeyFrame *, size_t>::iterator mit=obs.begin(), mend=obs.end(); mit!=mend; mit++)
    {
        KeyFrame *pKF = mit->first;
        if(!pMP->IsInKeyFrame(pKF))
        {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF,mit->second);
        }
        else
            pKF->EraseMapPointMatch(mit->second);
    }
    if(RecomputeOnReplace())
        pMP->ComputeDistinctiveDescriptors();
}

inline void MapPoint::ComputeDistinctiveDescriptors()
{
    if(mbBad || mObservations.empty())
        return;
    std::vector<std::pair<long unsigned int, const unsigned char *> > rows;
    for(std::map<KeyFrame *, size_t>::iterator mit=mObservations.begin(), mend=mObservations.end(); mit!=mend; mit++)
        if(!mit->first->isBad())
            rows.push_back(std::make_pair(mit->first->mnId, mit->first->mDescriptors.ptr((int)mit->second)));
    if(rows.empty())
        return;
    for(size_t i=1; i<rows.size(); i++)          // ascending mnId (insertion sort: a handful of observations)
        for(size_t j=i; j>0 && rows[j].first<rows[j-1].first; j--)
            std::swap(rows[j], rows[j-1]);
    const size_t N = rows.size();
    std::vector<std::vector<int> > Distances(N, std::vector<int>(N, 0));
    for(size_t i=0; i<N; i++)
        for(size_t j=i+1; j<N; j++)
        {
            int dist = 0;
            for(int b=0; b<32; b++)
                dist += __builtin_popcount((unsigned)(rows[i].second[b] ^ rows[j].second[b]));
            Distances[i][j] = Distances[j][i] = dist;
        }
    int BestMedian = 0x7FFFFFFF;
    size_t BestIdx = 0;
    for(size_t i=0; i<N; i++)
    {
        std::vector<int> vDists(Distances[i]);
        for(size_t a=1; a<N; a++)
            for(size_t b=a; b>0 && vDists[b]<vDists[b-1]; b--)
                std::swap(vDists[b], vDists[b-1]);
        const int median = vDists[(size_t)(0.5*(N-1))];
        if(median<BestMedian)
        {
            BestMedian = median;
            BestIdx = i;
        }
    }
    cv::Mat d(1, 32, CV_8U);
    for(int b=0; b<32; b++)
        d.ptr(0)[b] = rows[BestIdx].second[b];
    mDescriptor = d;
}

inline void MapPoint::UpdateNormalAndDepth()
{
    if(mbBad || mObservations.empty() || !mpRefKF)
        return;
    std::vector<std::pair<long unsigned int, KeyFrame *> > obs;
    for(std::map<KeyFrame *, size_t>::iterator mit=mObservations.begin(), mend=mObservations.end(); mit!=mend; mit++)
        obs.push_back(std::make_pair(mit->first->mnId, mit->first));
    for(size_t i=1; i<obs.size(); i++)           // ascending mnId
        for(size_t j=i; j>0 && obs[j].first<obs[j-1].first; j--)
            std::swap(obs[j], obs[j-1]);
    struct L2 {                                  // cv::norm(NORM_L2) of a CV_32F vector: summed in double, the root in double
        static double norm(const float d[3]) { return std::sqrt(((double)d[0]*d[0] + (double)d[1]*d[1]) + (double)d[2]*d[2]); }
    };
    const float P[3] = {mWorldPos.at<float>(0, 0), mWorldPos.at<float>(1, 0), mWorldPos.at<float>(2, 0)};
    float normal[3] = {0.f, 0.f, 0.f};
    for(size_t i=0; i<obs.size(); i++)
    {
        const cv::Mat Owi = obs[i].second->GetCameraCenter();
        const float d[3] = {P[0] - Owi.at<float>(0, 0), P[1] - Owi.at<float>(1, 0), P[2] - Owi.at<float>(2, 0)};
        const float a = (float)(1.0 / L2::norm(d));                 // normali/norm: a MatExpr scaled by alpha = 1.0/norm
        for(int c=0; c<3; c++)
        {
            const float t = d[c] * a;                               // normal + alpha*normali: scaleAdd on CV_32F
            normal[c] = t + normal[c];
        }
    }
    const cv::Mat Owr = mpRefKF->GetCameraCenter();
    const float PC[3] = {P[0] - Owr.at<float>(0, 0), P[1] - Owr.at<float>(1, 0), P[2] - Owr.at<float>(2, 0)};
    const float dist = (float)L2::norm(PC);
    const size_t idx = mObservations.count(mpRefKF) ? mObservations[mpRefKF] : 0;   // (the reference's operator[] reads 0 as well)
    const int level = mpRefKF->mvKeysUn[idx].octave;
    const float inv = (float)(1.0 / (double)obs.size());           // normal/n: convertTo with a float scale
    mfMaxDistance = dist * mpRefKF->mvScaleFactors[level];
    mfMinDistance = mfMaxDistance / mpRefKF->mvScaleFactors[mpRefKF->mnScaleLevels-1];
    cv::Mat nv(3, 1, CV_32F);
    for(int c=0; c<3; c++)
        nv.at<float>(c, 0) = normal[c] * inv;
    mNormalVector = nv;
}

inline void KeyFrame::OrderCovisibles(std::vector<std::pair<int, KeyFrame *> > &vPairs, std::vector<KeyFrame *> &vpKFs, std::vector<int> &vWs)
{
    struct ByWeightThenId {                      // ascending (weight, mnId)
        bool operator()(const std::pair<int, KeyFrame *> &a, const std::pair<int, KeyFrame *> &b) const
        {
            return a.first<b.first || (a.first==b.first && a.second->mnId<b.second->mnId);
        }
    };
    std::sort(vPairs.begin(), vPairs.end(), ByWeightThenId());
    vpKFs.clear();
    vWs.clear();
    for(size_t i=vPairs.size(); i>0; i--)        // push_front of each in turn
    {
        vpKFs.push_back(vPairs[i-1].second);
        vWs.push_back(vPairs[i-1].first);
    }
}

inline std::vector<KeyFrame *> KeyFrame::GetCovisiblesByWeight(const int &w)
{
    size_t n = 0;                                // mvOrderedWeights descends
    while(n<mvOrderedWeights.size() && mvOrderedWeights[n]>=w)
        n++;
    return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin()+n);
}

inline void KeyFrame::AddConnection(KeyFrame *pKF, const int &weight)
{
    if(!mConnectedKeyFrameWeights.count(pKF))
        mConnectedKeyFrameWeights[pKF]=weight;
    else if(mConnectedKeyFrameWeights[pKF]!=weight)
        mConnectedKeyFrameWeights[pKF]=weight;
    else
        return;
    UpdateBestCovisibles();
}

inline void KeyFrame::UpdateBestCovisibles()
{
    std::vector<std::pair<int, KeyFrame *> > vPairs;
    vPairs.reserve(mConnectedKeyFrameWeights.size());
    for(std::map<KeyFrame *, int>::iterator mit=mConnectedKeyFrameWeights.begin(), mend=mConnectedKeyFrameWeights.end(); mit!=mend; mit++)
        vPairs.push_back(std::make_pair(mit->second, mit->first));
    OrderCovisibles(vPairs, mvpOrderedConnectedKeyFrames, mvOrderedWeights);
}

inline void KeyFrame::UpdateConnections()
{
    std::map<KeyFrame *, int> KFcounter;
    const std::vector<MapPoint *> vpMP = mvpMapPoints;
    for(size_t i=0; i<vpMP.size(); i++)
    {
        MapPoint *pMP = vpMP[i];
        if(!pMP || pMP->isBad())
            continue;
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for(std::map<KeyFrame *, size_t>::const_iterator mit=observations.begin(), mend=observations.end(); mit!=mend; mit++)
        {
            if(mit->first->mnId==mnId)
                continue;
            KFcounter[mit->first]++;
        }
    }
    if(KFcounter.empty())
        return;

    const int th = 15;
    std::vector<std::pair<long unsigned int, KeyFrame *> > byId;   // the counter walked in ascending mnId
    for(std::map<KeyFrame *, int>::iterator mit=KFcounter.begin(), mend=KFcounter.end(); mit!=mend; mit++)
        byId.push_back(std::make_pair(mit->first->mnId, mit->first));
    std::sort(byId.begin(), byId.end());         // (mnId is unique)
    int nmax = 0;
    KeyFrame *pKFmax = NULL;
    std::vector<std::pair<int, KeyFrame *> > vPairs;
    for(size_t i=0; i<byId.size(); i++)
    {
        KeyFrame *pKFi = byId[i].second;
        const int w = KFcounter[pKFi];
        if(w>nmax)
        {
            nmax = w;
            pKFmax = pKFi;
        }
        if(w>=th)
        {
            vPairs.push_back(std::make_pair(w, pKFi));
            pKFi->AddConnection(this, w);
        }
    }
    if(vPairs.empty())
    {
        vPairs.push_back(std::make_pair(nmax, pKFmax));
        pKFmax->AddConnection(this, nmax);
    }
    mConnectedKeyFrameWeights = KFcounter;
    OrderCovisibles(vPairs, mvpOrderedConnectedKeyFrames, mvOrderedWeights);
    if(mbFirstConnection && mnId!=0)
    {
        mpParent = mvpOrderedConnectedKeyFrames.front();
        mpParent->AddChild(this);
        mbFirstConnection = false;
    }
}

}  // namespace ORB_SLAM2

#endif
