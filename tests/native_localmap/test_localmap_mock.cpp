// test_localmap_mock.cpp -- ORB_SLAM2::LocalMapSearch against a mock of the entry points it calls (mock_localmap.cc): what it
// sends (keys, raw distances, flags, the camera block, the skip byte, occupied) and what it does with the answer (member
// write-back, F.mvpMapPoints).  No device.  Prints "ok" and returns 0, or the failed checks.
#include <cstdio>
#include <cstring>

#include "LocalMap.h"
#include "hiperror.h"
#include "mock_localmap.h"

using namespace ORB_SLAM2;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_failed++; } \
    } while (0)

static MapPoint *point(float x, float y, float z, int nObs, bool bad, unsigned char fill)
{
    MapPoint *p = new MapPoint();
    p->mWorldPos = cv::Mat(3, 1, CV_32F);
    p->mNormalVector = cv::Mat(3, 1, CV_32F);
    p->mWorldPos.at<float>(0, 0) = x, p->mWorldPos.at<float>(1, 0) = y, p->mWorldPos.at<float>(2, 0) = z;
    p->mNormalVector.at<float>(0, 0) = -x, p->mNormalVector.at<float>(1, 0) = -y, p->mNormalVector.at<float>(2, 0) = -z;
    p->mfMinDistance = 1.5f + z, p->mfMaxDistance = 7.25f + z;
    p->mDescriptor = cv::Mat(1, 32, CV_8U);
    memset(p->mDescriptor.ptr(0), fill, 32);
    p->nObs = nObs;
    if (bad) p->SetBadFlag();
    return p;
}

int main()
{
    Frame::fx = 500, Frame::fy = 510, Frame::cx = 320, Frame::cy = 240;
    Frame::mnMinX = -3, Frame::mnMaxX = 650, Frame::mnMinY = -2, Frame::mnMaxY = 490;
    Frame::mfGridElementWidthInv = 64.f / 653.f, Frame::mfGridElementHeightInv = 48.f / 492.f;
    LocalMapSearch S(1000);
    CHECK(g_mock.maxPoints == 1000);

    // ---- Put / UpdateFlags / Erase / Clear ----
    std::vector<MapPoint *> P;
    P.push_back(point(1, 2, 3, 2, false, 0x11));      // 0: observed, will be in view
    P.push_back(point(4, 5, 6, 0, false, 0x22));      // 1: no observations, in view
    P.push_back(point(7, 8, 9, 1, true, 0x33));       // 2: bad
    P.push_back(point(1, 1, 1, 1, false, 0x44));      // 3: already seen in this frame (skip)
    P.push_back(point(2, 2, 2, 1, false, 0x55));      // 4: rejected by the frustum test
    S.Put(P);
    CHECK(g_mock.putKeys.size() == 5);
    for (int i = 0; i < 5; i++) CHECK(g_mock.putKeys[i] == P[i]->mnId + 1);
    CHECK(g_mock.putPos[3] == 4 && g_mock.putPos[4] == 5 && g_mock.putPos[5] == 6 && g_mock.putNormal[3] == -4);
    CHECK(g_mock.putMin[1] == 7.5f && g_mock.putMax[1] == 13.25f);      // the raw members, not 0.8f * / 1.2f *
    CHECK(g_mock.putDesc[32] == 0x22 && g_mock.putDesc[63] == 0x22 && g_mock.putDesc[64] == 0x33);
    CHECK(g_mock.putFlags[0] == ORBHIP_MP_OBSERVED && g_mock.putFlags[1] == 0 && g_mock.putFlags[2] == (ORBHIP_MP_OBSERVED | ORBHIP_MP_BAD));
    S.Put(P[1]);
    CHECK(g_mock.putKeys.size() == 1 && g_mock.putKeys[0] == P[1]->mnId + 1);
    P[1]->nObs = 3;
    S.UpdateFlags(P[1]);
    CHECK(g_mock.flagKeys.size() == 1 && g_mock.flagKeys[0] == P[1]->mnId + 1 && g_mock.flagVals[0] == ORBHIP_MP_OBSERVED);
    P[1]->nObs = 0;
    S.Erase(P[4]);
    CHECK(g_mock.erased.size() == 1 && g_mock.erased[0] == P[4]->mnId + 1);

    // ---- SearchLocalPoints ----
    Frame F;
    F.N = 4;
    F.mvKeysUn.resize(4);
    for (int i = 0; i < 4; i++) F.mvKeysUn[i].pt.x = 10.f * i, F.mvKeysUn[i].octave = i;
    F.mDescriptors = cv::Mat(4, 32, CV_8U);
    for (int i = 0; i < 4; i++) memset(F.mDescriptors.ptr(i), 0xA0 + i, 32);
    F.mvuRight.assign(4, -1.f);
    F.mvuRight[2] = 17.5f;
    F.mbf = 40.f;
    F.mnScaleLevels = 3;
    F.mvScaleFactors.push_back(1.f), F.mvScaleFactors.push_back(1.2f), F.mvScaleFactors.push_back(1.44f);
    F.mfLogScaleFactor = 0.18232156f;
    F.mTcw = cv::Mat::zeros(4, 4, CV_32F);
    // R = rotation by 90 degrees about z, t = (1, 2, 3): Ow = -R' t = (-2, 1, -3)
    F.mTcw.at<float>(0, 1) = -1, F.mTcw.at<float>(1, 0) = 1, F.mTcw.at<float>(2, 2) = 1, F.mTcw.at<float>(3, 3) = 1;
    F.mTcw.at<float>(0, 3) = 1, F.mTcw.at<float>(1, 3) = 2, F.mTcw.at<float>(2, 3) = 3;
    MapPoint *old0 = point(0, 0, 1, 1, false, 0), *old1 = point(0, 0, 1, 0, false, 0), *old3 = point(0, 0, 1, 2, false, 0);
    F.mvpMapPoints.assign(4, static_cast<MapPoint *>(NULL));
    F.mvpMapPoints[0] = old0, F.mvpMapPoints[1] = old1, F.mvpMapPoints[3] = old3;
    P[3]->mnLastFrameSeen = F.mnId;
    for (int i = 0; i < 5; i++) {      // stale values that the call must leave alone where the reference does
        P[i]->mnLastFrameSeen = i == 3 ? F.mnId : F.mnId + 7;
        P[i]->mbTrackInView = true, P[i]->mTrackProjX = 900 + i, P[i]->mTrackProjY = 800 + i, P[i]->mTrackProjXR = 700 + i;
        P[i]->mnTrackScaleLevel = 5, P[i]->mTrackViewCos = 0.25f;
    }
    const orbhip_local_point a0 = {101.f, 102.f, 93.f, 0.75f, 2, 1}, a1 = {201.f, 202.f, 193.f, 0.999f, 1, 1}, zero = {0, 0, 0, 0, 0, 0};
    g_mock.answerPoints = {a0, a1, zero, zero, zero};
    g_mock.answerMatch = {-1, 1, 0, -1};     // feature 1 <- point 1, feature 2 <- point 0
    g_mock.answerToMatch = 2, g_mock.answerMatches = 2;
    int toMatch = -1;
    const int found = S.SearchLocalPoints(F, P, 3.f, 0.5f, &toMatch);
    CHECK(found == 2 && toMatch == 2 && g_mock.searches == 1);
    // the frame became a resident set with a grid under mnId + 1
    CHECK(g_mock.setPuts == 1 && g_mock.setKey == F.mnId + 1 && g_mock.frameKey == F.mnId + 1 && g_mock.setN == 4 && g_mock.setNg == 0);
    CHECK(g_mock.setKps[2].x == 20.f && g_mock.setKps[3].octave == 3 && g_mock.setDesc[32 * 3] == 0xA3);
    CHECK(g_mock.grid[0] == -3 && g_mock.grid[1] == -2 && g_mock.grid[2] == Frame::mfGridElementWidthInv && g_mock.grid[3] == Frame::mfGridElementHeightInv);
    // the camera block
    const orbhip_local_camera &C = g_mock.cam;
    CHECK(C.Rcw[1] == -1 && C.Rcw[3] == 1 && C.Rcw[8] == 1 && C.Rcw[0] == 0 && C.tcw[0] == 1 && C.tcw[1] == 2 && C.tcw[2] == 3);
    CHECK(C.Ow[0] == -2 && C.Ow[1] == 1 && C.Ow[2] == -3);
    CHECK(C.fx == 500 && C.fy == 510 && C.cx == 320 && C.cy == 240 && C.mbf == 40);
    CHECK(C.min_x == -3 && C.max_x == 650 && C.min_y == -2 && C.max_y == 490);
    CHECK(C.nlevels == 3 && C.scale_factors[1] == 1.2f && C.scale_factors[2] == 1.44f && C.scale_factors[3] == 0 && C.log_scale_factor == 0.18232156f);
    CHECK(C.viewing_cos_limit == 0.5f && C.th == 3.f && g_mock.nnratio == 0.8f);
    // keys in list order, the skip byte, occupied = holds a point with observations, u_right
    for (int i = 0; i < 5; i++) CHECK(g_mock.keys[i] == P[i]->mnId + 1 && g_mock.skip[i] == (i == 3 ? 1 : 0));
    CHECK(g_mock.occupied[0] == 1 && g_mock.occupied[1] == 0 && g_mock.occupied[2] == 0 && g_mock.occupied[3] == 1);
    CHECK(g_mock.hadURight && g_mock.uRight[2] == 17.5f && g_mock.uRight[0] == -1.f);
    // write-back: in view -> all six members
    CHECK(P[0]->mbTrackInView && P[0]->mTrackProjX == 101.f && P[0]->mTrackProjY == 102.f && P[0]->mTrackProjXR == 93.f &&
          P[0]->mnTrackScaleLevel == 2 && P[0]->mTrackViewCos == 0.75f);
    CHECK(P[1]->mbTrackInView && P[1]->mTrackProjX == 201.f && P[1]->mnTrackScaleLevel == 1 && P[1]->mTrackViewCos == 0.999f);
    // rejected by the frustum test: mbTrackInView false, the other five as they were
    CHECK(!P[4]->mbTrackInView && P[4]->mTrackProjX == 904 && P[4]->mTrackProjY == 804 && P[4]->mTrackProjXR == 704 &&
          P[4]->mnTrackScaleLevel == 5 && P[4]->mTrackViewCos == 0.25f);
    // bad and skipped points: untouched, mbTrackInView included
    CHECK(P[2]->mbTrackInView && P[2]->mTrackProjX == 902 && P[3]->mbTrackInView && P[3]->mTrackProjX == 903 && P[3]->mnTrackScaleLevel == 5);
    // F.mvpMapPoints: match >= 0 overwrites, -1 leaves what was there
    CHECK(F.mvpMapPoints[0] == old0 && F.mvpMapPoints[1] == P[1] && F.mvpMapPoints[2] == P[0] && F.mvpMapPoints[3] == old3);
    // the same frame again: no second upload
    g_mock.answerMatch = {-1, -1, -1, -1};
    S.SearchLocalPoints(F, P, 1.f, 0.5f, &toMatch);
    CHECK(g_mock.setPuts == 1 && g_mock.searches == 2 && g_mock.cam.th == 1.f);
    CHECK(g_mock.occupied[1] == 0 && g_mock.occupied[2] == 1);      // P[1] has no observations, P[0] has
    // a frame without features: frame key 0, no set; an empty list: no call
    Frame E;
    E.mnScaleLevels = 3, E.mvScaleFactors = F.mvScaleFactors, E.mfLogScaleFactor = F.mfLogScaleFactor;
    E.mTcw = F.mTcw;
    g_mock.setN = 0;
    S.SearchLocalPoints(E, P, 1.f, 0.5f, &toMatch);
    CHECK(g_mock.frameKey == 0 && g_mock.setPuts == 1 && g_mock.searches == 3 && !g_mock.hadURight);
    CHECK(S.SearchLocalPoints(F, std::vector<MapPoint *>(), 1.f, 0.5f, &toMatch) == 0 && toMatch == 0 && g_mock.searches == 3);
    // a library error: reported, 0, nothing written
    g_mock.failSearch = true;
    g_mock.setKey = F.mnId + 1, g_mock.setN = 4;
    P[0]->mTrackProjX = 555.f;
    const unsigned long before = OrbHipErrorCount();
    toMatch = -1;
    CHECK(S.SearchLocalPoints(F, P, 1.f, 0.5f, &toMatch) == 0 && toMatch == 0 && OrbHipErrorCount() == before + 1);
    CHECK(P[0]->mTrackProjX == 555.f && F.mvpMapPoints[1] == P[1]);
    S.Clear();
    CHECK(g_mock.cleared == 1 && g_mock.dropped.size() == 1 && g_mock.dropped[0] == 0);
    if (!g_failed) printf("ok\n");
    return g_failed ? 1 : 0;
}
