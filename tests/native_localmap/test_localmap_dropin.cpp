// test_localmap_dropin.cpp -- ORB_SLAM2::LocalMapSearch::SearchLocalPoints against the host restatement of the reference's
// second loop of Tracking::SearchLocalPoints (ref: src/Tracking.cc:2336-2364: Frame::isInFrustum, src/Frame.cc:613-669, then the
// existing drop-in ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)) on the same scene, built twice as
// Frame / MapPoint objects: every tracking member of every point and F.mvpMapPoints must be equal.
//   test_localmap_dropin scene.bin            compares; prints "ok nToMatch nmatches" (exit 0) or the differences (exit 1)
//   test_localmap_dropin scene.bin bench R    times R calls of each path (tools/localmap_latency.py); microseconds per call
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "LocalMap.h"
#include "ORBmatcher.h"
#include "hiperror.h"

using namespace ORB_SLAM2;

struct Head {
    int32_t n, nq, nlevels, hasRight;
    float fx, fy, cx, cy, mbf, minX, maxX, minY, maxY, logS, th, limit;
    float Tcw[16];
    float sf[16];
};
struct PointRec {
    float pos[3], normal[3], minDist, maxDist;
};

struct World {
    Frame F;
    std::vector<MapPoint *> pts, held;
    float R[9], t[3], Ow[3];
};

static void build(World &W, const Head &H, const unsigned char *p)
{
    Frame &F = W.F;
    F.N = H.n;
    F.mvKeysUn.resize(H.n);
    memcpy(F.mvKeysUn.data(), p, (size_t)H.n * sizeof(cv::KeyPoint));
    p += (size_t)H.n * 28;
    F.mDescriptors = cv::Mat(H.n, 32, CV_8U);
    for (int i = 0; i < H.n; i++) memcpy(F.mDescriptors.ptr(i), p + (size_t)i * 32, 32);
    p += (size_t)H.n * 32;
    F.mvuRight.assign(H.n, -1.f);
    if (H.hasRight) memcpy(F.mvuRight.data(), p, (size_t)H.n * 4);
    p += (size_t)H.n * 4;
    const unsigned char *occ = p;
    p += H.n;
    F.mvpMapPoints.assign(H.n, static_cast<MapPoint *>(NULL));
    for (int i = 0; i < H.n; i++)
        if (occ[i]) {                       // a point the frame already holds: 1 = with observations, 2 = without
            MapPoint *m = new MapPoint();
            m->nObs = occ[i] == 1 ? 2 : 0;
            W.held.push_back(m);
            F.mvpMapPoints[i] = m;
        }
    F.mbf = H.mbf;
    F.mnScaleLevels = H.nlevels;
    F.mfLogScaleFactor = H.logS;
    F.mvScaleFactors.assign(H.sf, H.sf + H.nlevels);
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = H.Tcw[4 * r + c];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) W.R[3 * r + c] = H.Tcw[4 * r + c];
        W.t[r] = H.Tcw[4 * r + 3];
    }
    for (int r = 0; r < 3; r++) {           // mOw = -mRcw.t()*mtcw (ref: Frame::UpdatePoseMatrices), one gemm
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)W.R[3 * k + r] * (double)W.t[k];
        W.Ow[r] = (float)(-1.0 * s);
    }
    const PointRec *rec = (const PointRec *)p;
    p += (size_t)H.nq * sizeof(PointRec);
    const unsigned char *pd = p, *fl = p + (size_t)H.nq * 32, *skip = fl + H.nq;
    for (int k = 0; k < H.nq; k++) {
        MapPoint *m = new MapPoint();
        m->mWorldPos = cv::Mat(3, 1, CV_32F);
        m->mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int j = 0; j < 3; j++) m->mWorldPos.at<float>(j, 0) = rec[k].pos[j], m->mNormalVector.at<float>(j, 0) = rec[k].normal[j];
        m->mfMinDistance = rec[k].minDist, m->mfMaxDistance = rec[k].maxDist;
        m->mDescriptor = cv::Mat(1, 32, CV_8U);
        memcpy(m->mDescriptor.ptr(0), pd + (size_t)k * 32, 32);
        m->nObs = (fl[k] & 1) ? 3 : 0;
        if (fl[k] & 2) m->SetBadFlag();
        m->mnLastFrameSeen = skip[k] ? F.mnId : F.mnId + 1000;
        // stale tracking members: what the loops do not write must survive
        m->mbTrackInView = (k % 3) == 0, m->mTrackProjX = 1000.f + k, m->mTrackProjY = 2000.f + k, m->mTrackProjXR = 3000.f + k;
        m->mnTrackScaleLevel = k % 8, m->mTrackViewCos = 0.125f;
        W.pts.push_back(m);
    }
}

// Frame::isInFrustum (ref: src/Frame.cc:613-669) with OpenCV 2.4's evaluation of each cv::Mat expression
static bool isInFrustum(World &W, MapPoint *pMP, float viewingCosLimit)
{
    pMP->mbTrackInView = false;
    const cv::Mat Pm = pMP->GetWorldPos();
    const float P[3] = {Pm.at<float>(0, 0), Pm.at<float>(1, 0), Pm.at<float>(2, 0)};
    float Pc[3];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)W.R[3 * r + k] * (double)P[k];
        Pc[r] = (float)(s + (double)W.t[r]);
    }
    const float &PcX = Pc[0], &PcY = Pc[1], &PcZ = Pc[2];
    if(PcZ<0.0f)
        return false;
    const float invz = 1.0f/PcZ;
    const float u=Frame::fx*PcX*invz+Frame::cx;
    const float v=Frame::fy*PcY*invz+Frame::cy;
    if(u<Frame::mnMinX || u>Frame::mnMaxX)
        return false;
    if(v<Frame::mnMinY || v>Frame::mnMaxY)
        return false;
    const float maxDistance = pMP->GetMaxDistanceInvariance();
    const float minDistance = pMP->GetMinDistanceInvariance();
    const float PO[3] = {P[0] - W.Ow[0], P[1] - W.Ow[1], P[2] - W.Ow[2]};
    double sq = 0;
    for (int k = 0; k < 3; k++) sq += (double)PO[k] * (double)PO[k];
    const float dist = std::sqrt(sq);
    if(dist<minDistance || dist>maxDistance)
        return false;
    const cv::Mat Pn = pMP->GetNormal();
    double dot = 0;
    for (int k = 0; k < 3; k++) dot += (double)PO[k] * (double)Pn.at<float>(k, 0);
    const float viewCos = dot/dist;
    if(viewCos<viewingCosLimit)
        return false;
    const int nPredictedLevel = pMP->PredictScale(dist,&W.F);
    pMP->mbTrackInView = true;
    pMP->mTrackProjX = u;
    pMP->mTrackProjXR = u - W.F.mbf*invz;
    pMP->mTrackProjY = v;
    pMP->mnTrackScaleLevel= nPredictedLevel;
    pMP->mTrackViewCos = viewCos;
    return true;
}

static int hostLoop(World &W, float limit)
{
    int nToMatch = 0;
    for (size_t k = 0; k < W.pts.size(); k++) {
        MapPoint *pMP = W.pts[k];
        if(pMP->mnLastFrameSeen == W.F.mnId)
            continue;
        if(pMP->isBad())
            continue;
        if(isInFrustum(W, pMP, limit))
            nToMatch++;
    }
    return nToMatch;
}

static int referencePath(World &W, float th, float limit, int *nToMatch)
{
    *nToMatch = hostLoop(W, limit);
    if (*nToMatch == 0) return 0;
    ORBmatcher matcher(0.8);
    return matcher.SearchByProjection(W.F, W.pts, th);
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> buf(len);
    if (fread(buf.data(), 1, len, f) != (size_t)len) return 2;
    fclose(f);
    Head H;
    memcpy(&H, buf.data(), sizeof H);
    Frame::fx = H.fx, Frame::fy = H.fy, Frame::cx = H.cx, Frame::cy = H.cy;
    Frame::mnMinX = H.minX, Frame::mnMaxX = H.maxX, Frame::mnMinY = H.minY, Frame::mnMaxY = H.maxY;
    Frame::mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / (H.maxX - H.minX);
    Frame::mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / (H.maxY - H.minY);
    World A, B;
    build(A, H, buf.data() + sizeof H);
    build(B, H, buf.data() + sizeof H);
    LocalMapSearch S(1 << 16);
    S.Put(A.pts);

    if (argc >= 4 && !strcmp(argv[2], "bench")) {
        typedef std::chrono::steady_clock Clock;
        const int R = atoi(argv[3]);
        const std::vector<MapPoint *> heldA = A.F.mvpMapPoints, heldB = B.F.mvpMapPoints;
        std::vector<double> tRef, tNew, tNewPut, tLoop;
        int ntm = 0;
        ORBmatcher matcher(0.8);
        for (int it = 0; it < R + 20; it++) {     // 20 warm-up rounds; the paths alternate so that drift hits all alike
            B.F.mvpMapPoints = heldB;
            Clock::time_point t0 = Clock::now();
            ntm = hostLoop(B, H.limit);
            Clock::time_point t1 = Clock::now();
            if (ntm > 0) matcher.SearchByProjection(B.F, B.pts, H.th);
            Clock::time_point t2 = Clock::now();
            A.F.mvpMapPoints = heldA;
            Clock::time_point t3 = Clock::now();
            S.SearchLocalPoints(A.F, A.pts, H.th, H.limit, &ntm);
            Clock::time_point t4 = Clock::now();
            A.F.mvpMapPoints = heldA;
            A.F.mnId += 2000;                      // a frame the store has not seen: its upload is part of the call
            for (size_t k = 0; k < A.pts.size(); k++)
                if (A.pts[k]->mnLastFrameSeen == A.F.mnId - 2000) A.pts[k]->mnLastFrameSeen = A.F.mnId;
            Clock::time_point t5 = Clock::now();
            S.SearchLocalPoints(A.F, A.pts, H.th, H.limit, &ntm);
            Clock::time_point t6 = Clock::now();
            if (it < 20) continue;
            tLoop.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            tRef.push_back(std::chrono::duration<double, std::micro>(t2 - t0).count());
            tNew.push_back(std::chrono::duration<double, std::micro>(t4 - t3).count());
            tNewPut.push_back(std::chrono::duration<double, std::micro>(t6 - t5).count());
        }
        std::vector<double> *all[4] = {&tLoop, &tRef, &tNew, &tNewPut};
        const char *name[4] = {"host_loop", "per_call_path", "new_resident_frame", "new_with_frame_upload"};
        for (int j = 0; j < 4; j++) {
            std::sort(all[j]->begin(), all[j]->end());
            const size_t m = all[j]->size();
            printf("%s median %.1f p10 %.1f p90 %.1f\n", name[j], (*all[j])[m / 2], (*all[j])[m / 10], (*all[j])[m * 9 / 10]);
        }
        printf("n_to_match %d nq %d n %d\n", ntm, H.nq, H.n);
        // what LocalMapping pays per touched point: one upload, one launch, one synchronisation each
        std::vector<double> tFlags, tPut, tErase;
        for (int it = 0; it < R + 20; it++) {
            MapPoint *p = A.pts[(size_t)it % A.pts.size()];
            Clock::time_point t0 = Clock::now();
            S.UpdateFlags(p);
            Clock::time_point t1 = Clock::now();
            S.Erase(p);
            Clock::time_point t2 = Clock::now();
            S.Put(p);
            Clock::time_point t3 = Clock::now();
            if (it < 20) continue;
            tFlags.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            tErase.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
            tPut.push_back(std::chrono::duration<double, std::micro>(t3 - t2).count());
        }
        Clock::time_point b0 = Clock::now();
        S.Put(A.pts);
        const double tBatch = std::chrono::duration<double, std::micro>(Clock::now() - b0).count();
        std::vector<double> *one[3] = {&tFlags, &tErase, &tPut};
        const char *oneName[3] = {"update_flags_one", "erase_one", "put_one"};
        for (int j = 0; j < 3; j++) {
            std::sort(one[j]->begin(), one[j]->end());
            const size_t m = one[j]->size();
            printf("%s median %.1f p10 %.1f p90 %.1f\n", oneName[j], (*one[j])[m / 2], (*one[j])[m / 10], (*one[j])[m * 9 / 10]);
        }
        printf("put_all %d points %.1f\n", H.nq, tBatch);
        return OrbHipErrorCount() ? 1 : 0;
    }

    int ntmA = -1, ntmB = -1;
    const int foundA = S.SearchLocalPoints(A.F, A.pts, H.th, H.limit, &ntmA);
    const int foundB = referencePath(B, H.th, H.limit, &ntmB);
    int bad = 0;
    if (foundA != foundB || ntmA != ntmB) { printf("counts differ: %d/%d matches, %d/%d to match\n", foundA, foundB, ntmA, ntmB); bad++; }
    for (int k = 0; k < H.nq; k++) {
        MapPoint *a = A.pts[k], *b = B.pts[k];
        if (a->mbTrackInView != b->mbTrackInView || !same_bits(a->mTrackProjX, b->mTrackProjX) || !same_bits(a->mTrackProjY, b->mTrackProjY) ||
            !same_bits(a->mTrackProjXR, b->mTrackProjXR) || a->mnTrackScaleLevel != b->mnTrackScaleLevel ||
            !same_bits(a->mTrackViewCos, b->mTrackViewCos)) {
            if (bad++ < 10) printf("point %d differs: inView %d/%d u %.9g/%.9g level %d/%d\n", k, (int)a->mbTrackInView, (int)b->mbTrackInView,
                                   a->mTrackProjX, b->mTrackProjX, a->mnTrackScaleLevel, b->mnTrackScaleLevel);
        }
    }
    for (int i = 0; i < H.n; i++) {
        // the same point of the local map, the same held point (by position in the held list), or NULL on both sides
        MapPoint *a = A.F.mvpMapPoints[i], *b = B.F.mvpMapPoints[i];
        const long ia = a ? std::find(A.pts.begin(), A.pts.end(), a) - A.pts.begin() : -1;
        const long ib = b ? std::find(B.pts.begin(), B.pts.end(), b) - B.pts.begin() : -1;
        const long ha = a ? std::find(A.held.begin(), A.held.end(), a) - A.held.begin() : -1;
        const long hb = b ? std::find(B.held.begin(), B.held.end(), b) - B.held.begin() : -1;
        if (ia != ib || ha != hb)
            if (bad++ < 10) printf("feature %d holds point %ld/%ld (held %ld/%ld)\n", i, ia, ib, ha, hb);
    }
    if (OrbHipErrorCount()) { printf("drop-in error: %s\n", OrbHipLastError()); bad++; }
    if (!bad) printf("ok %d %d\n", ntmA, foundA);
    return bad ? 1 : 0;
}
