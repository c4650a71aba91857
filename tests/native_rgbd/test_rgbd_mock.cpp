// Frame::ComputeStereoFromRGBD (host/rgbd/FrameRGBD.cc) against a mock of the one entry point it calls: what it passes on (the
// distorted and the undistorted keypoints, the map's type, size and step, the factor, mbf), and what it leaves when the call
// fails -- every keypoint without a depth and one hipdetail::Fail record, no exception.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hiperror.h"
#include "orbhip.h"
#include "slamlite.h"

static int g_calls = 0, g_fail = 0;
static struct { const void *kps, *kun, *depth; int n, type, dw, dh, stride; float factor, mbf; } g_seen;

extern "C" const char *orbhip_last_error(const orbhip_ctx *) { return "mock: refused"; }
extern "C" int orbhip_rgbd_depth(orbhip_ctx *, const orbhip_keypoint *kps, const orbhip_keypoint *kun, int n, const void *depth, int type,
                                 int dw, int dh, int stride, float factor, float mbf, float *ur, float *dz)
{
    g_calls++;
    g_seen = {kps, kun, depth, n, type, dw, dh, stride, factor, mbf};
    for (int i = 0; i < n; i++) { ur[i] = 10.0f + i; dz[i] = 20.0f + i; }     // (written even when failing: the caller must wipe it)
    return g_fail ? ORBHIP_E_ARG : ORBHIP_OK;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    using namespace ORB_SLAM2;
    Frame F;
    F.N = 5;
    F.mvKeys.resize(5);
    F.mvKeysUn.resize(5);
    F.mbf = 40.0f;
    cv::Mat raw(12, 20, CV_16UC1), conv(12, 20, CV_32FC1);
    cv::Mat roi = cv::Mat(cv::Mat(12, 24, CV_16UC1), cv::Rect(2, 1, 20, 10));      // a view with a step

    F.ComputeStereoFromRGBD(raw, 0.0002f);
    CHECK(g_calls == 1 && g_seen.kps == F.mvKeys.data() && g_seen.kun == F.mvKeysUn.data() && g_seen.n == 5);
    CHECK(g_seen.depth == raw.data && g_seen.type == ORBHIP_DEPTH_U16 && g_seen.dw == 20 && g_seen.dh == 12 && g_seen.stride == 40);
    CHECK(g_seen.factor == 0.0002f && g_seen.mbf == 40.0f);
    CHECK(F.mvuRight.size() == 5 && F.mvDepth.size() == 5 && F.mvuRight[4] == 14.0f && F.mvDepth[0] == 20.0f);

    F.ComputeStereoFromRGBD(conv);                               // the reference's signature: a converted map, factor 1
    CHECK(g_calls == 2 && g_seen.type == ORBHIP_DEPTH_F32 && g_seen.stride == 80 && g_seen.factor == 1.0f && g_seen.depth == conv.data);
    F.ComputeStereoFromRGBD(roi, 0.5f);
    CHECK(g_calls == 3 && g_seen.depth == roi.data && g_seen.dw == 20 && g_seen.dh == 10 && g_seen.stride == 48);

    // a type the library does not read is passed on as an unknown depth type, for the library to refuse
    cv::Mat bytes(12, 20, CV_8UC1);
    F.ComputeStereoFromRGBD(bytes, 1.0f);
    CHECK(g_calls == 4 && g_seen.type != ORBHIP_DEPTH_U16 && g_seen.type != ORBHIP_DEPTH_F32 && g_seen.type != ORBHIP_DEPTH_NONE);

    // failure: all -1, one record, nothing thrown
    const unsigned long before = OrbHipErrorCount();
    g_fail = 1;
    F.ComputeStereoFromRGBD(raw, 0.0002f);
    CHECK(g_calls == 5 && OrbHipErrorCount() == before + 1);
    CHECK(std::string(OrbHipLastError()).find("ComputeStereoFromRGBD") != std::string::npos);
    CHECK(std::string(OrbHipLastError()).find("mock: refused") != std::string::npos);
    for (int i = 0; i < 5; i++) CHECK(F.mvuRight[i] == -1.0f && F.mvDepth[i] == -1.0f);
    g_fail = 0;

    // keypoint vectors that do not match N: refused before the library is called; no features: nothing to do
    F.mvKeysUn.resize(4);
    F.ComputeStereoFromRGBD(raw, 0.0002f);
    CHECK(g_calls == 5 && OrbHipErrorCount() == before + 2 && F.mvDepth.size() == 5 && F.mvDepth[2] == -1.0f);
    F.N = 0; F.mvKeys.clear(); F.mvKeysUn.clear();
    F.ComputeStereoFromRGBD(raw, 0.0002f);
    CHECK(g_calls == 5 && OrbHipErrorCount() == before + 2 && F.mvuRight.empty() && F.mvDepth.empty());
    printf("ok\n");
    return 0;
}
