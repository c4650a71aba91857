// test_localcollect.cpp -- ORB_SLAM2::LocalMapSearch::UpdateLocalMap against a host restatement of Tracking::UpdateLocalMap
// (ref: src/Tracking.cc:2377-2562, keyframeCounter and the children walked in ascending mnId order: the canonical order of
// docs/parity.md) on the same mock KeyFrame / MapPoint objects, over a map that grows, fuses, replaces and culls points and
// loses key frames between frames.  vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF, F.mvpMapPoints and every
// mnTrackReferenceForFrame stamp must be equal.  Links either the host model of the entry points (mock_collect.cc) or
// liborbhip.  Prints "ok <frames> <key frames> <points> <largest local map>" and returns 0, or the failed checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "LocalMap.h"
#include "hiperror.h"
#include "ref_update_local_map.h"

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static unsigned g_seed = 12345;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }

using refrestate::ref_update;

struct World {
    LocalMapSearch &S;
    std::vector<KeyFrame *> kfs;      // in the map (bad ones included until they are erased)
    std::vector<MapPoint *> pts;      // in the map
    std::vector<KeyFrame *> allKfs;
    std::vector<MapPoint *> allPts;
    explicit World(LocalMapSearch &s) : S(s) {}

    MapPoint *new_point()
    {
        MapPoint *p = new MapPoint();
        p->mWorldPos = cv::Mat(3, 1, CV_32F), p->mNormalVector = cv::Mat(3, 1, CV_32F), p->mDescriptor = cv::Mat(1, 32, CV_8U);
        for (int k = 0; k < 3; k++) p->mWorldPos.at<float>(k, 0) = (float)rnd(100), p->mNormalVector.at<float>(k, 0) = 1.f;
        memset(p->mDescriptor.ptr(0), (int)rnd(256), 32);
        p->mfMinDistance = 1, p->mfMaxDistance = 10;
        pts.push_back(p), allPts.push_back(p);
        S.Put(p);
        return p;
    }
    MapPoint *live_point() { return pts.empty() ? NULL : pts[rnd((unsigned)pts.size())]; }

    void grow(int N, int nOld, int nNew)
    {
        KeyFrame *kf = new KeyFrame();
        kf->N = N;
        kf->mvpMapPoints.assign(N, (MapPoint *)NULL);
        std::vector<MapPoint *> touched;
        for (int k = 0; k < nOld + nNew; k++) {
            MapPoint *p = k < nOld ? live_point() : new_point();
            const int idx = (int)rnd(N);
            if (!p || p->isBad() || kf->mvpMapPoints[idx] || p->IsInKeyFrame(kf)) continue;
            kf->AddMapPoint(p, idx);
            p->AddObservation(kf, idx);
            touched.push_back(p);
        }
        if (rnd(3) == 0 && !touched.empty()) {   // a point twice in the vector: its observation names the first index only
            const int twin = (touched[0]->GetIndexInKeyFrame(kf) + 1) % N;
            if (!kf->mvpMapPoints[twin]) kf->mvpMapPoints[twin] = touched[0];
        }
        // the covisibility graph: key frames by shared points; the best one is the parent
        std::vector<std::pair<int, KeyFrame *> > w;
        for (size_t k = 0; k < kfs.size(); k++) {
            int shared = 0;
            for (size_t t = 0; t < touched.size(); t++) shared += touched[t]->IsInKeyFrame(kfs[k]) ? 1 : 0;
            if (shared) w.push_back(std::make_pair(-shared, kfs[k]));
        }
        std::sort(w.begin(), w.end(), [](const std::pair<int, KeyFrame *> &a, const std::pair<int, KeyFrame *> &b) {
            return a.first != b.first ? a.first < b.first : a.second->mnId < b.second->mnId;
        });
        for (size_t k = 0; k < w.size(); k++) {
            kf->mvpOrderedConnectedKeyFrames.push_back(w[k].second);
            w[k].second->mvpOrderedConnectedKeyFrames.insert(w[k].second->mvpOrderedConnectedKeyFrames.begin(), kf);
        }
        if (!w.empty()) kf->mpParent = w[0].second, w[0].second->mspChildrens.insert(kf);
        kfs.push_back(kf), allKfs.push_back(kf);
        for (size_t t = 0; t < touched.size(); t++) S.UpdateFlags(touched[t]);
        S.PutKeyFrame(kf);
    }

    void forget(MapPoint *p)
    {
        pts.erase(std::find(pts.begin(), pts.end(), p));
        S.Erase(p);
    }

    // ORBmatcher::Fuse / LoopClosing: a is replaced by b (ref: src/MapPoint.cc:192-230)
    void replace(MapPoint *a, MapPoint *b)
    {
        if (!a || !b || a == b || a->isBad() || b->isBad()) return;
        const std::map<KeyFrame *, size_t> obs = a->GetObservations();
        std::vector<std::pair<std::pair<KeyFrame *, size_t>, bool> > moved;
        for (std::map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); it++)
            moved.push_back(std::make_pair(*it, !b->IsInKeyFrame(it->first)));
        a->Replace(b);
        for (size_t k = 0; k < moved.size(); k++) S.SetMapPoint(moved[k].first.first, moved[k].first.second, moved[k].second ? b : NULL);
        S.UpdateFlags(b);
        forget(a);
    }

    // MapPoint::SetBadFlag (ref: src/MapPoint.cc:157-183); half of the time the flag alone is set first and a frame sees the bad point
    void cull(MapPoint *p, bool flagOnly)
    {
        if (!p) return;
        p->SetBadFlag();
        if (flagOnly) return S.UpdateFlags(p);
        const std::map<KeyFrame *, size_t> obs = p->GetObservations();
        for (std::map<KeyFrame *, size_t>::const_iterator it = obs.begin(); it != obs.end(); it++) {
            it->first->EraseMapPointMatch(it->second);
            S.SetMapPoint(it->first, it->second, NULL);
        }
        p->mObservations.clear();
        p->nObs = 0;
        forget(p);
    }

    // KeyFrame::SetBadFlag (ref: src/KeyFrame.cc): its points lose the observation, the graph forgets it
    // returns whether the key frame left the map
    bool drop_kf(KeyFrame *kf, bool flagOnly)
    {
        kf->mbBad = true;
        if (flagOnly) return false;
        for (size_t i = 0; i < kf->mvpMapPoints.size(); i++) {
            MapPoint *p = kf->mvpMapPoints[i];
            if (p && p->GetIndexInKeyFrame(kf) == (int)i) {
                p->mObservations.erase(kf);
                p->nObs--;
                if (std::find(pts.begin(), pts.end(), p) != pts.end()) S.UpdateFlags(p);
            }
        }
        // the spanning tree and the graph forget it (ref: src/KeyFrame.cc SetBadFlag gives the children a new parent)
        for (std::set<KeyFrame *>::iterator it = kf->mspChildrens.begin(); it != kf->mspChildrens.end(); it++) {
            (*it)->mpParent = kf->mpParent;
            if (kf->mpParent) kf->mpParent->mspChildrens.insert(*it);
        }
        if (kf->mpParent) kf->mpParent->mspChildrens.erase(kf);
        for (size_t k = 0; k < allKfs.size(); k++) {
            std::vector<KeyFrame *> &v = allKfs[k]->mvpOrderedConnectedKeyFrames;
            v.erase(std::remove(v.begin(), v.end(), kf), v.end());
        }
        // (its mvpMapPoints stays as it is, as in the reference)
        kfs.erase(std::find(kfs.begin(), kfs.end(), kf));
        S.EraseKeyFrame(kf);
        return true;
    }
};

// The documented departure (include/orbhip/LocalMap.h): a frame that matched nothing keeps the last
// list; a key frame of that list that was erased meanwhile still gives its points to the reference's UpdateLocalPoints, and
// gives none to the class.  Both sides are checked against what they document.
static void erased_key_frame_adds_nothing(World &W)
{
    KeyFrame *gone = NULL;
    for (size_t k = W.kfs.size(); k-- > 0 && !gone;)   // the newest: most of its points are still in the map
        if (!W.kfs[k]->isBad()) gone = W.kfs[k];
    std::vector<KeyFrame *> list(1, gone);
    for (size_t k = W.kfs.size(); k-- > 0 && list.size() < 3;)
        if (W.kfs[k] != gone && !W.kfs[k]->isBad()) list.push_back(W.kfs[k]);
    std::vector<KeyFrame *> rest(list.begin() + 1, list.end());
    W.drop_kf(gone, false);
    Frame F, G, H;          // matched nothing: the vote is empty, the lists stay
    std::vector<KeyFrame *> a = list, b = list, c = rest;
    std::vector<MapPoint *> withGone, got, withoutGone;
    KeyFrame *ra = NULL, *rb = NULL, *rc = NULL;
    ref_update(F, a, withGone, ra);
    W.S.UpdateLocalMap(G, b, got, rb);
    ref_update(H, c, withoutGone, rc);
    CHECK(a == list && b == list && !ra && !rb);
    CHECK(got == withoutGone);
    CHECK(withGone.size() > withoutGone.size());
}

int main()
{
    Frame::fx = 500, Frame::fy = 510, Frame::cx = 320, Frame::cy = 240;
    Frame::mnMinX = 0, Frame::mnMaxX = 640, Frame::mnMinY = 0, Frame::mnMaxY = 480;
    Frame::mfGridElementWidthInv = 64.f / 640.f, Frame::mfGridElementHeightInv = 48.f / 480.f;
    LocalMapSearch S(8192);
    S.InitKeyFrames(128, 64);
    World W(S);
    Frame dummy;   // (a frame with mnId 0 would meet the stamps' initial value, in the reference as well)
    std::vector<KeyFrame *> refKFs, gotKFs;
    std::vector<MapPoint *> refMPs, gotMPs;
    KeyFrame *refRef = NULL, *gotRef = NULL;
    size_t largest = 0;
    int frames = 0;
    for (int step = 0; step < 120; step++) {
        W.grow(64, 20 + (int)rnd(20), 5 + (int)rnd(10));
        for (int k = 0; k < 3; k++) W.replace(W.live_point(), W.live_point());
        for (int k = 0; k < 2; k++) W.cull(W.live_point(), rnd(2) == 0);
        if (step % 9 == 8) {
            KeyFrame *gone = W.kfs[rnd((unsigned)W.kfs.size())];
            if (W.drop_kf(gone, rnd(2) == 0)) {
                // The one place where the class departs from the reference: an erased key frame adds no points even where the
                // list carried over from the last frame still names it (an empty vote keeps that list), while the reference
                // reads the mvpMapPoints its SetBadFlag leaves behind.  The oracle is NOT bent to that: the erased key frame
                // leaves both carried lists here, and erased_key_frame_adds_nothing() below checks the departure by itself.
                refKFs.erase(std::remove(refKFs.begin(), refKFs.end(), gone), refKFs.end());
                gotKFs.erase(std::remove(gotKFs.begin(), gotKFs.end(), gone), gotKFs.end());
            }
        }
        // a frame that matched points of the map: repeats, NULLs, bad points; every 13th frame matched nothing
        Frame F;
        F.N = 50;
        F.mvpMapPoints.assign(F.N, (MapPoint *)NULL);
        F.mvKeys.resize(F.N), F.mvKeysUn.resize(F.N);
        F.mDescriptors = cv::Mat(F.N, 32, CV_8U);
        for (int i = 0; i < F.N; i++) {
            F.mvKeysUn[i].pt.x = (float)(10 + rnd(600)), F.mvKeysUn[i].pt.y = (float)(10 + rnd(440)), F.mvKeysUn[i].octave = 0;
            memset(F.mDescriptors.ptr(i), (int)rnd(256), 32);
        }
        F.mnScaleLevels = 1, F.mfScaleFactor = 1.2f, F.mfLogScaleFactor = logf(1.2f);
        F.mvScaleFactors.assign(1, 1.0f);
        F.mTcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = r == c ? 1.f : 0.f;
        if (step % 13 != 12)
            for (int i = 0; i < F.N; i++) F.mvpMapPoints[i] = rnd(5) == 0 ? NULL : W.allPts[W.allPts.size() - 1 - rnd(std::min<unsigned>(80, (unsigned)W.allPts.size()))];
        for (int i = 0; i < F.N; i++)   // (points the map has forgotten are not in a frame: Tracking drops what Replace / SetBadFlag left)
            if (F.mvpMapPoints[i] && std::find(W.pts.begin(), W.pts.end(), F.mvpMapPoints[i]) == W.pts.end()) F.mvpMapPoints[i] = NULL;
        const std::vector<MapPoint *> frameBefore = F.mvpMapPoints;
        std::vector<long unsigned int> kfBefore(W.allKfs.size()), mpBefore(W.allPts.size()), kfStamp(W.allKfs.size()), mpStamp(W.allPts.size());
        for (size_t k = 0; k < W.allKfs.size(); k++) kfBefore[k] = W.allKfs[k]->mnTrackReferenceForFrame;
        for (size_t k = 0; k < W.allPts.size(); k++) mpBefore[k] = W.allPts[k]->mnTrackReferenceForFrame;
        ref_update(F, refKFs, refMPs, refRef);
        const std::vector<MapPoint *> frameRef = F.mvpMapPoints;
        // the same objects as they were, for the class under test
        for (size_t k = 0; k < W.allKfs.size(); k++) kfStamp[k] = W.allKfs[k]->mnTrackReferenceForFrame, W.allKfs[k]->mnTrackReferenceForFrame = kfBefore[k];
        for (size_t k = 0; k < W.allPts.size(); k++) mpStamp[k] = W.allPts[k]->mnTrackReferenceForFrame, W.allPts[k]->mnTrackReferenceForFrame = mpBefore[k];
        F.mvpMapPoints = frameBefore;
        S.UpdateLocalMap(F, gotKFs, gotMPs, gotRef);
        CHECK(gotKFs == refKFs);
        CHECK(gotMPs == refMPs);
        CHECK(gotRef == refRef);
        CHECK(F.mvpMapPoints == frameRef);
        for (size_t k = 0; k < W.allKfs.size(); k++) CHECK(W.allKfs[k]->mnTrackReferenceForFrame == kfStamp[k]);
        for (size_t k = 0; k < W.allPts.size(); k++) CHECK(W.allPts[k]->mnTrackReferenceForFrame == mpStamp[k]);
        std::vector<MapPoint *> fused;
        int ntm = -1;
        CHECK(S.TrackLocalPoints(F, gotKFs, fused, 1.0f, 0.5f, &ntm) >= 0 && fused == refMPs);
        largest = std::max(largest, refMPs.size());
        frames++;
        if (g_failed > 20) break;
    }
    CHECK(largest > 300 && W.kfs.size() > 80);
    erased_key_frame_adds_nothing(W);
    CHECK(OrbHipErrorCount() == 0);
    const int nkf = (int)W.kfs.size(), npts = (int)W.pts.size();
    for (size_t k = 0; k < W.allKfs.size(); k++) delete W.allKfs[k];
    for (size_t k = 0; k < W.allPts.size(); k++) delete W.allPts[k];
    if (g_failed) return printf("%d checks failed\n", g_failed), 1;
    printf("ok %d %d %d %d\n", frames, nkf, npts, (int)largest);
    return 0;
}
