// A drop-in Frame from an RGB image and a CV_16U depth map, the way Tracking::GrabImageRGBD and the Frame RGB-D constructor
// build one (ref: src/Tracking.cc:904-932, src/Frame.cc:463-516) with the three-line change of INTEGRATION.md 3f: the colour
// cv::Mat goes straight into ORBextractor::operator() (SetColorOrder), UndistortKeyPoints, then ComputeStereoFromRGBD on the raw
// map with the factor -- and, for comparison, on the float map the caller of this program converted.
//   test_rgbd_dropin <scene.bin> <out.bin>
// scene.bin: int32 w, h; float K[9], dist[5], bf, factor; w*h*3 RGB bytes; w*h uint16 depth; w*h float converted depth.
// out.bin: int32 n; n keypoints, n undistorted keypoints, n x 32 descriptor bytes, mvuRight, mvDepth (raw map), mvuRight,
// mvDepth (converted map), level 0 of mvImagePyramid (w*h bytes); the same keypoint count again from a frame-build run.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ORBextractor.h"
#include "hiperror.h"
#include "slamlite.h"

using namespace ORB_SLAM2;

static bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int wh[2];
    float par[16];
    if (!f || fread(wh, 4, 2, f) != 2 || fread(par, 4, 16, f) != 16) { perror(argv[1]); return 2; }
    const int w = wh[0], h = wh[1];
    std::vector<unsigned char> rgb((size_t)w * h * 3);
    std::vector<unsigned short> d16((size_t)w * h);
    std::vector<float> d32((size_t)w * h);
    if (fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || fread(d16.data(), 2, d16.size(), f) != d16.size() ||
        fread(d32.data(), 4, d32.size(), f) != d32.size()) { fprintf(stderr, "short scene file\n"); return 2; }
    fclose(f);
    const float bf = par[14], factor = par[15];

    cv::Mat imRGB(h, w, CV_8UC3, rgb.data()), imD(h, w, CV_16UC1, d16.data()), imDconv(h, w, CV_32FC1, d32.data());
    ORBextractor ex(1000, 1.2f, 8, 20, 7);
    ex.SetColorOrder(true);                                      // Camera.RGB: 1
    Frame F;
    F.mK = cv::Mat(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) F.mK.at<float>(i / 3, i % 3) = par[i];
    F.mDistCoef = cv::Mat(5, 1, CV_32F);
    for (int i = 0; i < 5; i++) F.mDistCoef.at<float>(i, 0) = par[9 + i];
    F.mbf = bf;
    F.mpORBextractorLeft = &ex;

    ex(imRGB, cv::Mat(), F.mvKeys, F.mDescriptors);              // ExtractORB on the colour frame
    F.N = (int)F.mvKeys.size();
    if (F.N == 0 || OrbHipErrorCount()) { fprintf(stderr, "extraction failed: %s\n", OrbHipLastError()); return 1; }
    F.UndistortKeyPoints();
    cv::Mat lvl0 = ex.mvImagePyramid[0].clone();
    if (lvl0.rows != h || lvl0.cols != w || lvl0.type() != CV_8UC1) { fprintf(stderr, "mvImagePyramid[0] is not the grey image\n"); return 1; }

    F.ComputeStereoFromRGBD(imD, factor);
    std::vector<float> ur1 = F.mvuRight, dz1 = F.mvDepth;
    F.ComputeStereoFromRGBD(imDconv);
    if (ur1.size() != (size_t)F.N || memcmp(ur1.data(), F.mvuRight.data(), 4 * ur1.size()) || memcmp(dz1.data(), F.mvDepth.data(), 4 * dz1.size()))
    { fprintf(stderr, "the raw map with its factor and the converted map disagree\n"); return 1; }

    // the same frame with the frame build armed: one graph launch, the same features, the undistorted keypoints as a by-product
    std::vector<cv::KeyPoint> keys2, un2;
    cv::Mat desc2;
    ex.SetFrameBuild(F.mK, F.mDistCoef, 0.0f, 0.0f, 64.0f / w, 48.0f / h);
    ex(imRGB, cv::Mat(), keys2, desc2);
    const bool built = ex.BuiltKeysUn(keys2, F.mK, F.mDistCoef, un2);
    if ((int)keys2.size() != F.N || memcmp(keys2.data(), F.mvKeys.data(), sizeof(cv::KeyPoint) * F.N) || !built ||
        memcmp(un2.data(), F.mvKeysUn.data(), sizeof(cv::KeyPoint) * F.N))
    { fprintf(stderr, "the frame build on the colour frame disagrees with the plain call (%d vs %d features, by-products %d)\n", (int)keys2.size(), F.N, (int)built); return 1; }
    if (OrbHipErrorCount()) { fprintf(stderr, "drop-in error: %s\n", OrbHipLastError()); return 1; }

    FILE *o = fopen(argv[2], "wb");
    bool ok = o && put(o, &F.N, 4) && put(o, F.mvKeys.data(), sizeof(cv::KeyPoint) * F.N) && put(o, F.mvKeysUn.data(), sizeof(cv::KeyPoint) * F.N);
    for (int i = 0; ok && i < F.N; i++) ok = put(o, F.mDescriptors.ptr(i), 32);
    ok = ok && put(o, ur1.data(), 4 * ur1.size()) && put(o, dz1.data(), 4 * dz1.size()) && put(o, F.mvuRight.data(), 4 * F.N) && put(o, F.mvDepth.data(), 4 * F.N);
    for (int y = 0; ok && y < h; y++) ok = put(o, lvl0.ptr(y), w);
    if (!ok || fclose(o)) { perror(argv[2]); return 2; }
    int with = 0;
    for (int i = 0; i < F.N; i++) with += dz1[i] > 0;
    printf("ok %d %d\n", F.N, with);
    return 0;
}
