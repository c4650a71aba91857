// LocalMap.h -- ORB_SLAM2::LocalMapSearch: the second half of Tracking::SearchLocalPoints (ref: src/Tracking.cc:2336-2364 --
// Frame::isInFrustum over mvpLocalMapPoints, then ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)) as one
// device call against map points that stay on the device (orbhip_map_*, orbhip_search_local_points; include/orbhip.h,
// DESIGN.md section 10).  No counterpart class in the reference: LocalMapping / LoopClosing tell it when a point changes (Put,
// UpdateFlags, Erase), Tracking calls SearchLocalPoints.  Never throws; a failed device call is
// reported through hipdetail::Fail and SearchLocalPoints returns 0 with nothing written (include/orbhip/hiperror.h).
#ifndef ORBHIP_LOCALMAP_H
#define ORBHIP_LOCALMAP_H

#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#ifdef ORBHIP_WITH_REFERENCE_HEADERS
#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#else
#include "slamlite.h"
#endif

struct orbhip_ctx;
struct orbhip_bow_candidate;

#ifndef ORBHIP_WITH_REFERENCE_HEADERS
#ifndef ORBHIP_CVLITE_POINT3F
#define ORBHIP_CVLITE_POINT3F
namespace cv
{
template <typename T> struct Point3_ {
    T x, y, z;
    Point3_() : x(0), y(0), z(0) {}
    Point3_(T _x, T _y, T _z) : x(_x), y(_y), z(_z) {}
};
typedef Point3_<float> Point3f;
}  // namespace cv
#endif
#endif

namespace ORB_SLAM2
{

// What PnPsolver::PnPsolver(F, vpMapPointMatches) and the mvMaxError loop of SetRansacParameters build for one candidate key frame
// (ref: src/PnPsolver.cc:78-101, :154-156), in the form RansacScore::ScorePnP takes: one entry per frame feature that holds a
// matched point, in ascending feature index.  Empty for a candidate below minMatches.
struct RelocCorrespondences
{
    std::vector<cv::Point2f> mvP2D;
    std::vector<float> mvMaxError;               // mvSigma2[i] * th2
    std::vector<cv::Point3f> mvP3Dw;
    std::vector<size_t> mvKeyPointIndices;
};

class LocalMapSearch
{
public:
    // a store for at most maxPoints map points, in a device context of its own (a context is not re-entrant)
    explicit LocalMapSearch(int maxPoints = 1 << 20);
    ~LocalMapSearch();
    LocalMapSearch(const LocalMapSearch &) = delete;
    LocalMapSearch &operator=(const LocalMapSearch &) = delete;

    // The point's position, normal, distance range, descriptor and flags as they are now (key MapPoint::mnId + 1): after
    // SetWorldPos, UpdateNormalAndDepth, ComputeDistinctiveDescriptors, and for every new point.  The vector form is one upload.
    void Put(MapPoint *pMP);
    void Put(const std::vector<MapPoint *> &vpMPs);
    // Observations() > 0 and isBad() alone: after AddObservation / EraseObservation / SetBadFlag
    void UpdateFlags(MapPoint *pMP);
    // after Replace and at the end of SetBadFlag
    void Erase(MapPoint *pMP);
    // from Tracking::Reset (with ClearKeyFrames() where key frames are kept here as well)
    void Clear();

    // Leaves F.mvpMapPoints and, for every point of vpLocalMapPoints that is neither bad nor already seen in this frame
    // (mnLastFrameSeen == F.mnId), mbTrackInView / mTrackProjX / mTrackProjY / mTrackProjXR / mnTrackScaleLevel /
    // mTrackViewCos exactly as the reference's loop and SearchByProjection leave them.  IncreaseVisible() stays with the caller
    // (for the points with mbTrackInView).  *nToMatch = the number of points in view; returns the number of matches.
    int SearchLocalPoints(Frame &F, const std::vector<MapPoint *> &vpLocalMapPoints, float th, float viewingCosLimit,
                          int *nToMatch);

    // ---- Tracking::UpdateLocalMap on the device (orbhip_map_kf_*, orbhip_map_vote, orbhip_map_collect,
    // orbhip_track_local_points) ----
    // Room for maxKFs key frames of at most maxRow features; before the first PutKeyFrame (which otherwise takes 4096 x 2048).
    void InitKeyFrames(int maxKFs, int maxRow);
    // pKF->mvpMapPoints as it is now (key KeyFrame::mnId + 1): for every new key frame.  Of a point the vector holds twice
    // only the index GetIndexInKeyFrame reports is kept; points that were never Put are left out.
    void PutKeyFrame(KeyFrame *pKF);
    // one entry: after AddMapPoint / ReplaceMapPointMatch (pMP) and EraseMapPointMatch (NULL)
    void SetMapPoint(KeyFrame *pKF, size_t idx, MapPoint *pMP);
    // at the end of KeyFrame::SetBadFlag.  From then on the key frame adds no points to a local map, also where a list made
    // before still names it (the reference would read the mvpMapPoints that SetBadFlag leaves in the bad key frame).
    void EraseKeyFrame(KeyFrame *pKF);
    // from Tracking::Reset, beside Clear(): forgets every key frame and frees the table's rows
    void ClearKeyFrames();
    // UpdateLocalKeyFrames alone (vote + covisibility step), for a caller that goes on with TrackLocalPoints
    void UpdateLocalKeyFrames(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, KeyFrame *&pReferenceKF);
    // Tracking::UpdateLocalMap without SetReferenceMapPoints: the vote on the device, the covisibility step of
    // UpdateLocalKeyFrames here on the caller's objects with keyframeCounter walked in ascending mnId order (the reference
    // walks it by heap address) and children in ascending mnId order, UpdateLocalPoints on the device.  Leaves the three
    // outputs, F.mvpMapPoints (bad points become NULL) and the mnTrackReferenceForFrame stamps as the reference does; when no
    // key frame shares a point with F, vpLocalKeyFrames and pReferenceKF stay and the points are rebuilt from them, as there.
    void UpdateLocalMap(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints,
                        KeyFrame *&pReferenceKF);
    // UpdateLocalPoints and the second half of SearchLocalPoints as one device call: vpLocalMapPoints is rebuilt from
    // vpLocalKeyFrames and searched; the points of F.mvpMapPoints with mnLastFrameSeen == F.mnId are skipped.  Everything
    // else as SearchLocalPoints.
    int TrackLocalPoints(Frame &F, const std::vector<KeyFrame *> &vpLocalKeyFrames, std::vector<MapPoint *> &vpLocalMapPoints, float th,
                         float viewingCosLimit, int *nToMatch);

    // ---- Tracking's other two projection searches on the resident map (orbhip_search_last_frame,
    // orbhip_search_keyframe_points) ----
    // ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) of TrackWithMotionModel (ref: src/ORBmatcher.cc:
    // 1341-1498): the same return value, and Cur.mvpMapPoints written the same way -- the last point assigned to a feature
    // stays, a feature whose match the rotation check removed becomes NULL, every other feature is left alone.  Both frames
    // become resident sets the first time they are searched.  Points of Last that were never Put (Tracking's temporal stereo
    // points) are put before the call, with one upload; the caller Erases them when it deletes them.
    int SearchLastFrame(Frame &Cur, const Frame &Last, float th, bool bMono, bool checkOri = true);
    // ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) of Relocalization (ref: :1500-1627).  The
    // key frame's points are those of its row in the table (PutKeyFrame / SetMapPoint; put here when it has none yet): equal
    // to pKF->GetMapPointMatches() under the rule PutKeyFrame states.  Returns and writes as SearchLastFrame.
    int SearchKeyFramePoints(Frame &Cur, KeyFrame *pKF, const std::set<MapPoint *> &sAlreadyFound, float th, int ORBdist,
                             bool checkOri = true);

    // ---- ORBmatcher::Fuse for LocalMapping::SearchInNeighbors on the resident map (orbhip_fuse_row, orbhip_fuse_collect;
    // DESIGN.md section 17) ----
    // The first loop of SearchInNeighbors (ref: src/LocalMapping.cc:2549-2556): matcher.Fuse(pKFi, pKF->GetMapPointMatches(), th)
    // for every pKFi of vpTargetKFs, in that order, with the same map edits (AddObservation / AddMapPoint / Replace) and the same
    // return values, one per target.  All targets are projected and searched in one device call (64 targets at a time beyond
    // that); the results are then applied target by target and point by point, re-reading isBad(), IsInKeyFrame() and what the
    // feature holds at that moment, and a point whose descriptor changed because it survived a Replace in an earlier target is
    // searched again, with its new descriptor, before a later target is applied.  pKF's points are those of its row in the table
    // (put here when it has none yet) and must have been Put; the targets' features become resident sets the first time.
    std::vector<int> FuseInTargets(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th = 3.0);
    // The second loop (ref: :2558-2581): vpFuseCandidates = the points of vpTargetKFs, each once, bad ones left out, fused into
    // pKF with matcher.Fuse(pKF, vpFuseCandidates, th).  The union is built on the device and never leaves it except as the list
    // the results are applied to.  Returns Fuse's return value.
    int FuseCandidates(KeyFrame *pKF, const std::vector<KeyFrame *> &vpTargetKFs, float th = 3.0);
    // Both bring the resident state up to date with every edit they make: the rows of the key frames a replaced point was
    // observed in, its flags, the survivor's descriptor and flags, the row entry and the flags of an added observation.

    // ---- LoopClosing's two projection searches on the resident map (orbhip_search_loop_points, orbhip_fuse_sim3,
    // orbhip_map_kf_set_batch) ----
    // LoopClosing::ComputeSim3 from "Retrieve MapPoints seen in Loop Keyframe and neighbors" on (ref: src/LoopClosing.cc:404-427):
    // vpLoopMapPoints is filled element for element from the rows of vpLoopConnectedKFs (in that order; bad points and second
    // occurrences left out), projected with Scw into pCurrentKF and matched as ORBmatcher::SearchByProjection(pCurrentKF, Scw,
    // vpLoopMapPoints, vpCurrentMatchedPoints, th) does (ref: src/ORBmatcher.cc:290-403): vpCurrentMatchedPoints gains the new
    // matches, the return value is theirs.  The union never leaves the device except as the list itself.  The stamp
    // mnLoopPointForKF is not written: nothing else reads it.
    int SearchLoopPoints(KeyFrame *pCurrentKF, const cv::Mat &Scw, const std::vector<KeyFrame *> &vpLoopConnectedKFs,
                         std::vector<MapPoint *> &vpLoopMapPoints, std::vector<MapPoint *> &vpCurrentMatchedPoints, int th);
    // LoopClosing::SearchAndFuse (ref: src/LoopClosing.cc:647-673): matcher.Fuse(pKF, Scw, vpLoopMapPoints, th, vpReplacePoints)
    // and the Replace loop behind it for every (key frame, corrected similarity) of vCorrectedPoses, in the vector's order (the
    // reference walks a map<KeyFrame*, ...> by heap address; docs/parity.md).  All targets are projected and searched in one
    // device call (64 at a time beyond that); the results are applied target by target, re-reading isBad(), GetMapPoints() and
    // what the feature holds at that moment, and a loop point whose descriptor changed because it survived a Replace in an
    // earlier target is searched again before a later target is applied.  Points that CorrectLoop moved must be current in the
    // store: CorrectLoopPoints below leaves them so.
    void SearchAndFuse(const std::vector<std::pair<KeyFrame *, cv::Mat> > &vCorrectedPoses, const std::vector<MapPoint *> &vpLoopMapPoints,
                       float th = 4);
    // where SearchAndFuse spends its time, in microseconds, summed over the calls since the caller last zeroed it
    // (tools/loopfuse_latency.py): preparation, device call, second searches, apply and Replace loops, resident state
    struct LoopPhases { double prepare, device, research, apply, resident; };
    static LoopPhases &Phases() { static LoopPhases p = {0, 0, 0, 0, 0}; return p; }
    // for the tests: without the second search of changed survivors the result differs from the reference's
    static bool &ResearchChangedSurvivors() { static bool b = true; return b; }

    // ---- ORBmatcher::SearchBySim3 on the resident map (orbhip_search_by_sim3) ----
    // matcher.SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) of LoopClosing::ComputeSim3 (ref: src/ORBmatcher.cc:1102-1326,
    // src/LoopClosing.cc:375): the same return value and the same edits to vpMatches12.  Both key frames' points are those of
    // their rows in the table, both feature sets become resident the first time; the two projections, the two window searches
    // and the agreement are one device call, and vpMatches12[i1] = pKF2->GetMapPointMatches()[i2] for the agreed pairs.  Returns
    // -1 with vpMatches12 untouched -- the caller then runs ORBmatcher::SearchBySim3 -- when a key frame has no row (PutKeyFrame),
    // when a key frame holds a non-NULL, non-bad point that was never Put, or when the device call fails (hiperror.h).
    int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches12, const float &s12, const cv::Mat &R12,
                     const cv::Mat &t12, const float th);

    // ---- map points refreshed in place on the resident store (orbhip_map_refresh) ----
    // The loops "pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth();" over a key frame's points (ref:
    // src/LocalMapping.cc:2036-2046, :2577-2590; the UpdateNormalAndDepth loops of src/Optimizer.cc with bDescriptors = false) as one
    // device call: the lists are built from GetObservations() in ascending KeyFrame::mnId, the observers' features become resident
    // sets (in ascending mnId, up to the set limit in force), and mDescriptor / mNormalVector / mfMinDistance / mfMaxDistance are
    // assigned from what the call wrote into the store.  A point with an observer beyond the set limit, one that was never Put, or
    // one whose mpRefKF is not among its observers goes the host way: the per-point methods, then one Put of all of them.  NULL
    // entries, bad points, points without observations and second occurrences in vpMPs are skipped, as the reference's loop skips
    // them.  The scale pyramid (mvScaleFactors, mnScaleLevels) is that of the first observer: one per SLAM session.  Returns the
    // number of points touched: every point of vpMPs that was not skipped.
    int RefreshPoints(const std::vector<MapPoint *> &vpMPs, bool bDescriptors = true, bool bNormals = true);
    // how many points the RefreshPoints calls of this process sent each way (for the tests and tools/refresh_latency.py)
    struct RefreshWays { long device, host; };
    static RefreshWays &RefreshCounts() { static RefreshWays w = {0, 0}; return w; }
    // ---- the covisibility graph from the resident key-frame table (orbhip_map_covis; DESIGN.md section 20, INTEGRATION.md
    // section 3e) ----
    // KeyFrame::UpdateConnections (ref: src/KeyFrame.cc:731-843) for one key frame or for a batch: one device call counts the
    // points every key frame of vpKFs shares with every key frame of the table, then the key frames are updated in the vector's
    // order exactly as sequential pKF->UpdateConnections() calls would -- mConnectedKeyFrameWeights assigned, AddConnection on
    // every neighbour of weight >= 15 (or on the single maximum), the two ordered lists assigned, the parent set on a key frame's
    // first connection (mnId != 0).  The counts do not depend on that order: UpdateConnections edits neither points nor rows.
    // Orders the reference takes from heap addresses are taken from mnId (docs/parity.md).  A key frame without a row is put.
    // Precondition: every key frame that observes one of the points has its row in the table (PutKeyFrame for every new key
    // frame); an erased key frame is nobody's neighbour.  A key frame that holds a non-NULL, non-bad point the store does not
    // know goes the host way: pKF->UpdateConnections() itself.
    // With pLoopConnections, what LoopClosing::CorrectLoop does per key frame (ref: src/LoopClosing.cc:600-616):
    // (*pLoopConnections)[pKF] = the key frames of mConnectedKeyFrameWeights after the update, minus
    // GetVectorCovisibleKeyFrames() from before it, minus *pvpExclude (mvpCurrentConnectedKFs).
    void UpdateConnections(KeyFrame *pKF);
    void UpdateConnections(const std::vector<KeyFrame *> &vpKFs, std::map<KeyFrame *, std::set<KeyFrame *> > *pLoopConnections = 0,
                           const std::vector<KeyFrame *> *pvpExclude = 0);
    // how many key frames the UpdateConnections calls of this process sent each way (for the tests and tools/covis_latency.py)
    struct CovisWays { long device, host; };
    static CovisWays &CovisCounts() { static CovisWays w = {0, 0}; return w; }

    // ---- SearchByBoW against all candidate key frames in one call (orbhip_search_by_bow_candidates; DESIGN.md section 21,
    // INTEGRATION.md section 3e) ----
    // The loop of Tracking::Relocalization (ref: src/Tracking.cc:2595-2616): matcher.SearchByBoW(pKF, F, vvpMapPointMatches[i]) for
    // every candidate, matcher = ORBmatcher(nnratio, checkOri).  vvpMapPointMatches[i] and vnMatches[i] are what the call leaves and
    // returns; a candidate with isBad() gets an empty vector and 0.  With pvSetups, (*pvSetups)[i] holds what the PnPsolver
    // constructor and SetRansacParameters(.., th2) would gather for every candidate with vnMatches[i] >= minMatches.  All candidates
    // are matched in one device call (as many as the set limit allows beyond that): the key frames' features are resident sets
    // (put here the first time), "has a point that is not bad" is read from their rows of the table, the positions from the store.
    // Indices are turned back into MapPoint* from GetMapPointMatches() at the moment of application.  A candidate that holds a
    // non-NULL, non-bad point the store does not know goes the host way, through ORBmatcher::SearchByBoW and the host loop.
    void SearchByBoWCandidates(const std::vector<KeyFrame *> &vpCandidateKFs, Frame &F, std::vector<std::vector<MapPoint *> > &vvpMapPointMatches,
                               std::vector<int> &vnMatches, std::vector<RelocCorrespondences> *pvSetups = 0, int minMatches = 15,
                               float th2 = 5.991, float nnratio = 0.75, bool checkOri = true);
    // The loop of LoopClosing::ComputeSim3 (ref: src/LoopClosing.cc:304-332): matcher.SearchByBoW(pCurrentKF, pKF, vvpMatches12[i]) for
    // every candidate.  When pCurrentKF holds a point the store does not know, every candidate goes the host way.
    void SearchByBoWCandidates(KeyFrame *pCurrentKF, const std::vector<KeyFrame *> &vpCandidateKFs,
                               std::vector<std::vector<MapPoint *> > &vvpMatches12, std::vector<int> &vnMatches, float nnratio = 0.75,
                               bool checkOri = true);
    // how many candidates the SearchByBoWCandidates calls of this process sent each way (for the tests and tools/bowcand_latency.py)
    struct BowCandWays { long device, host; };
    static BowCandWays &BowCandCounts() { static BowCandWays w = {0, 0}; return w; }

    // ---- LocalMapping::KeyFrameCulling on the resident map (orbhip_map_kf_levels, orbhip_map_cull; DESIGN.md section 22,
    // INTEGRATION.md section 3e) ----
    // The counting loop of KeyFrameCulling and KeyFrameCullingForMonoVI (ref: src/LocalMapping.cc:2705-2753, :1533-1581) for every
    // key frame of vpKFs on the map as it is now: vCounts[k] = nMPs, nRedundantObservations and nRedundantObservations>0.9*nMPs of
    // vpKFs[k].  One device call; before it, the octave / stereo / far byte of every feature (mvKeysUn, mvuRight, mvDepth against
    // mThDepth) is uploaded, once per key frame, for the rows that have none yet.  A batch is not the sequence: SetBadFlag of one
    // key frame changes Observations() of its points and can turn them bad, so these counts hold until the first cull and no longer
    // (KeyFrameCulling below counts again).  A key frame without a row is put.  Precondition as UpdateConnections': every observer's
    // row is in the table and current, flags are current.  A key frame that holds a non-NULL, non-bad point the store does not know,
    // or that is bad itself, goes the host way: the reference's loop on the objects.  false = nothing filled (a device error,
    // reported through hipdetail::Fail).
    struct CullCount { int nMPs, nRedundant; bool bRedundant; };
    bool CullCounts(const std::vector<KeyFrame *> &vpKFs, bool bMonocular, std::vector<CullCount> &vCounts);
    // after the caller's pKF->SetBadFlag(): EraseKeyFrame(pKF), and one UpdateFlags upload for those of vpItsPoints (the key
    // frame's GetMapPointMatches() from before the call) that are bad now
    void KeyFrameCulled(KeyFrame *pKF, const std::vector<MapPoint *> &vpItsPoints);
    // The whole loop over vpLocalKeyFrames, in the vector's order, with the reference's result: for every key frame but mnId == 0,
    // skip(pKF) is asked at that moment (the VI variant's tests read GetPrevKeyFrame() / GetNextKeyFrame(), which an earlier cull
    // relinks); a redundant one is culled through cull(pKF) -- the caller's pKF->SetBadFlag() -- and KeyFrameCulled, and the
    // candidates behind it are counted again before the next verdict.  Device calls: culls + 1 at the most.  Returns the number
    // culled; after a device error nothing more is culled.
    template <class Skip, class Cull>
    int KeyFrameCulling(const std::vector<KeyFrame *> &vpLocalKeyFrames, bool bMonocular, Skip skip, Cull cull)
    {
        std::vector<CullCount> vCounts;
        size_t nFirst = 0;        // vCounts[i - nFirst] is vpLocalKeyFrames[i]'s
        bool bCurrent = false;    // no cull since vCounts was made
        int nCulled = 0;
        for (size_t i = 0; i < vpLocalKeyFrames.size(); i++) {
            KeyFrame *pKF = vpLocalKeyFrames[i];
            if (pKF->mnId == 0) continue;
            if (skip(pKF)) continue;
            if (!bCurrent) {
                if (!CullCounts(std::vector<KeyFrame *>(vpLocalKeyFrames.begin() + i, vpLocalKeyFrames.end()), bMonocular, vCounts)) return nCulled;
                nFirst = i;
                bCurrent = true;
            }
            if (!vCounts[i - nFirst].bRedundant) continue;
            const std::vector<MapPoint *> vpItsPoints = pKF->GetMapPointMatches();
            cull(pKF);
            KeyFrameCulled(pKF, vpItsPoints);
            bCurrent = false;
            nCulled++;
        }
        return nCulled;
    }
    // how many key frames the CullCounts calls of this process sent each way (for the tests and tools/cull_latency.py)
    struct CullWays { long device, host; };
    static CullWays &CullWayCounts() { static CullWays w = {0, 0}; return w; }

    // ---- the set-up of local bundle adjustment from the resident key-frame table (orbhip_map_ba_problem; DESIGN.md section 24,
    // INTEGRATION.md section 3e) ----
    // What Optimizer::LocalBundleAdjustment forms before the solver sees a vertex (ref: src/Optimizer.cc:2772-2820, :2888 ff.), in one
    // device call instead of two copies of every local point's observation map:
    //   vpLocalKFs   the local key frames, as given or as BuildLocalBA forms them
    //   vpLocalMPs   lLocalMapPoints, in the reference's order
    //   vpFixedKFs   lFixedCameras: the observers of a local point that are no local key frame, in the order of the reference's walk
    //                with ascending mnId standing for the order of map<KeyFrame*, size_t> (docs/parity.md)
    //   vEdgeOff, vEdges   the observations of vpLocalMPs[j] are vEdges[vEdgeOff[j] .. vEdgeOff[j + 1]), ascending mnId: one per
    //                edge the reference adds.  The caller reads pKF->mvKeysUn[idx] and pKF->mvuRight[idx] itself.
    // Indices become pointers at the moment of application.  Both calls leave mnBALocalForKF / mnBAFixedForKF on the objects as the
    // reference does.  Precondition as UpdateConnections': every observer's row is in the table and current, flags are current, a
    // key frame that turned bad has been erased.  false = a failed device call, or a local key frame without a row: `out` is
    // empty and the caller runs its own loops (the hiperror.h convention).
    struct BAEdge { KeyFrame *pKF; size_t idx; };
    struct BAProblem {
        std::vector<KeyFrame *> vpLocalKFs, vpFixedKFs;
        std::vector<MapPoint *> vpLocalMPs;
        std::vector<int32_t> vEdgeOff;
        std::vector<BAEdge> vEdges;
    };
    // forms the list of :2772-2784 itself: pKF and its GetVectorCovisibleKeyFrames(), every one stamped with pKF->mnId, the bad
    // ones stamped but not listed
    bool BuildLocalBA(KeyFrame *pKF, BAProblem &out);
    // a caller-given window (LocalBundleAdjustmentNavState, :980 ff.; the other LocalBundleAdjustment, :1720 ff.), or every key
    // frame for BundleAdjustment (:2358 ff.): NULL and bad key frames are left out, the stamp is vpLocalKFs.back()->mnId (the
    // window's pCurKF).  The key frame before the window, which the windowed forms fix as well, is the caller's to add.
    bool BuildBAProblem(const std::vector<KeyFrame *> &vpLocalKFs, BAProblem &out);

    // ---- map points moved in place on the resident store (orbhip_map_correct_sim3, orbhip_map_correct_se3; DESIGN.md section 23,
    // INTEGRATION.md section 3e) ----
    // A g2o::Sim3 as the call reads it: rotation().coeffs() (x y z w), translation(), scale().  The Sim3 algebra -- the composition
    // g2oSic*mg2oScw, inverse(), the quaternion from Riw -- stays with the caller, who holds the g2o objects.
    struct Sim3d { double q[4], t[3], s; };
    // one iteration of CorrectLoop's loop over CorrectedSim3: the key frame, NonCorrectedSim3[pKF], CorrectedSim3[pKF].inverse() and
    // the pose the loop sets at its end (Converter::toCvSE3(eigR, eigt/s))
    struct LoopCorrection { KeyFrame *pKF; Sim3d Siw, correctedSwi; cv::Mat correctedTiw; };
    // The point loop and the SetPose of LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-564) as one device call.  The vector's
    // order stands for the iteration order of the reference's map<KeyFrame*, g2o::Sim3> (docs/parity.md).  Every key frame's
    // GetMapPointMatches() is walked in order; NULL entries, bad points and points already stamped with nCurrentKFid are skipped, so
    // the first key frame to reach a point owns it.  A point is stamped (mnCorrectedByKF, mnCorrectedReference), mapped through Siw
    // and correctedSwi in double and refreshed as MapPoint::UpdateNormalAndDepth would at that moment of the sequence: observers
    // earlier in the vector stand at their corrected centres, the others where they stood.  Position, normal and distance range are
    // assigned to the objects from what the call wrote into the store; then SetPose(correctedTiw) runs on every key frame in order.
    // A point that was never Put, or whose mpRefKF is not among its observers, goes the host way at its turn in the sequence and is
    // Put afterwards.  pKF->UpdateConnections() stays with the caller (UpdateConnections above).  Returns the number of points moved.
    int CorrectLoopPoints(const std::vector<LoopCorrection> &v, unsigned long nCurrentKFid);
    // The point loop of LoopClosing::RunGlobalBundleAdjustment (ref: :765-797) over vpMPs (Map::GetAllMapPoints(): each point once;
    // NULL entries, bad points and second occurrences are skipped), after the caller has set mTcwBefGBA and the new pose of every
    // adjusted key frame: a point with mnBAGlobalForKF == nLoopKF takes mPosGBA, another is carried from its reference key frame's
    // mTcwBefGBA to its GetPoseInverse(); a point whose reference key frame was not adjusted is left alone.  One device call; the
    // positions are assigned to the objects.  A point that was never Put goes the host way and is Put.  Returns the number moved.
    int ApplyGlobalBA(const std::vector<MapPoint *> &vpMPs, unsigned long nLoopKF);
    // how many points the two calls of this process sent each way (for the tests and tools/correct_latency.py)
    struct CorrectWays { long device, host; };
    static CorrectWays &CorrectCounts() { static CorrectWays w = {0, 0}; return w; }
    // where the two calls spend their time, in microseconds, summed since the caller last zeroed it (tools/correct_latency.py):
    // building the lists, the entry point, assigning the results (with the host way and SetPose)
    struct CorrectPhases { double prepare, device, apply; };
    static CorrectPhases &CorrectTimes() { static CorrectPhases p = {0, 0, 0}; return p; }

    // orbhip_set_limit for this object's context: how many key-frame sets stay resident (4 .. 96; 96 from the first Fuse or
    // Refresh call on unless set here).  Returns the limit in force.
    int SetLimit(int maxSets);

    // device of the objects constructed from now on (default 0)
    static void SetDevice(int device);

protected:
    bool PutLocked(const std::vector<MapPoint *> &vpMPs);      // Put / PutKeyFrame with mMutex held
    bool PutKeyFrameLocked(KeyFrame *pKF);
    bool EnsureKeyFrames();
    bool VoteAndGraph(Frame &F, std::vector<KeyFrame *> &vpLocalKeyFrames, KeyFrame *&pReferenceKF);
    bool CollectKeys(const std::vector<KeyFrame *> &vpKFs, std::vector<uint64_t> &kfKeys);
    // ---- the steps the LocalMap*.cc files share, one definition each, all with mMutex held ----
    // The store's side (LocalMap.cc): key -> object or NULL; was the point Put; was every non-NULL, non-bad point of the list (else
    // its key frame goes the host way); keys -> objects element for element; keys and flags of these points in one call.
    MapPoint *PointOf(uint64_t key) const;
    bool Known(MapPoint *pMP) const;
    bool AllKnown(const std::vector<MapPoint *> &vpMPs) const;
    void PointsOf(const uint64_t *keys, int n, std::vector<MapPoint *> &out) const;
    bool UpdateFlagsLocked(MapPoint *const *points, size_t n, const char *who);
    static void AssignNormalDepth(MapPoint *pMP, const float *nrm, float minDistance, float maxDistance);   // a member: the reference protects all three
    // The table's side (LocalMapCollect.cc).  A row is a key frame's when the table holds one under its key AND for this object: two
    // live KeyFrame objects never share an mnId, since the device row is addressed by mnId + 1 whatever the host map says.
    KeyFrame *KeyFrameOf(uint64_t key) const;
    bool HasRow(KeyFrame *pKF) const;
    bool EnsureRow(KeyFrame *pKF) { return HasRow(pKF) || PutKeyFrameLocked(pKF); }
    bool EraseKeyFrameLocked(KeyFrame *pKF, const char *who);     // false: there is no table, nothing was done
    // Fuse's apply loop over one target (ref: src/ORBmatcher.cc:951-972) and the resident state behind it (LocalMapFuse.cc)
    struct FuseEdits {
        std::set<MapPoint *> put, flags;
        std::map<MapPoint *, std::vector<unsigned char> > survivors; // of a Replace: the descriptor each had at the device call
        std::set<std::pair<KeyFrame *, size_t> > entries;           // (key frame, feature) whose row entry may have changed
        void Remember(MapPoint *surv);                              // keeps a survivor's descriptor, once
        bool ChangedSince(MapPoint *pMP) const;                     // a survivor whose descriptor differs from the remembered one
        void Replace(MapPoint *dead, MapPoint *surv);               // dead->Replace(surv), noting the rows, flags and put it dirties
    };
    int ApplyFuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMPs, const int32_t *bestIdx, const int32_t *bestDist, FuseEdits &edits);
    bool FlushFuse(FuseEdits &edits);
    typedef std::map<uint64_t, std::pair<std::vector<int32_t>, std::vector<uint64_t> > > FuseRows;
    bool TakeFuseEdits(FuseEdits &edits, FuseRows &rows);         // what the two flushes share: the store's half, the table's as lists
    bool FlushLoop(FuseEdits &edits);                             // FlushFuse with one orbhip_map_kf_set_batch (LocalMapLoop.cc)
    bool EnsureFuseSet(KeyFrame *pKF, uint64_t *setKey);
    bool ResidentKeyFrame(KeyFrame *pKF, uint64_t *setKey);       // SearchByBoWCandidates: row and set of a key frame the store knows (LocalMapBowCand.cc)
    void SortCandidates(const std::vector<KeyFrame *> &vpKFs, bool device, std::vector<int> &way, std::vector<orbhip_bow_candidate> &cand,
                        std::vector<size_t> &who);                // SearchByBoWCandidates: which way each candidate goes
    bool BuildBALocked(const std::vector<KeyFrame *> &vpLocalKFs, unsigned long nStamp, BAProblem &out);   // LocalMapBA.cc

    orbhip_ctx *mpCtx;
    std::mutex mMutex;
    std::unordered_map<uint64_t, MapPoint *> mPointOf;   // key -> the object, for the lists that come back as keys
    std::map<uint64_t, KeyFrame *> mKeyFrameOf;
    bool mbKeyFrames = false;
    size_t mnLastVoted = 0, mnLastLocal = 0;   // sizes of the last answers: how much room the next call offers first
    size_t mnLastCandidates = 0, mnLastLoopPoints = 0;
    size_t mnLastLinks = 0;                    // links per key frame of the last UpdateConnections, rounded up
    size_t mnLastBAEdges = 0, mnLastBAFixed = 0;   // of the last BuildLocalBA / BuildBAProblem
    bool mbFuseSets = false;                  // the set limit has been raised for the targets of FuseInTargets
    int mnSetLimit = 4;                        // the set limit in force (orbhip_set_limit)
};

}  // namespace ORB_SLAM2

#endif
