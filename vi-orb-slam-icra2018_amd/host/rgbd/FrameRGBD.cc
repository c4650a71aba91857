// FrameRGBD.cc -- Frame::ComputeStereoFromRGBD (ref: src/Frame.cc:987-1008) through liborbhip: the depth under every keypoint
// and the virtual right coordinate, mvuRight = mvKeysUn.x - mbf / d.  The overload with a factor takes the map as the sensor
// delivers it (CV_16U or CV_32F) and does what imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) (ref: src/Tracking.cc:924-925)
// would have done, at those pixels only.  Host arithmetic inside the library, no device work; no exception (hiperror.h): on an
// error no keypoint gets a depth.
#include "hiperror.h"
#include "orbhip.h"
#include "ORBextractor.h"
#include "slamlite.h"

namespace ORB_SLAM2
{

void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth)
{
    ComputeStereoFromRGBD(imDepth, 1.0f);                        // a converted map: CV_32F, used as it is
}

void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepthRaw, float depthMapFactor)
{
    mvuRight.assign(N, -1.0f);                                   // ref: :989-990
    mvDepth.assign(N, -1.0f);
    if (N == 0) return;
    if ((int)mvKeys.size() != N || (int)mvKeysUn.size() != N)
    {
        hipdetail::Fail("Frame::ComputeStereoFromRGBD", "mvKeys / mvKeysUn do not hold N keypoints");
        return;
    }
    const int type = imDepthRaw.type() == CV_16UC1 ? ORBHIP_DEPTH_U16 : imDepthRaw.type() == CV_32FC1 ? ORBHIP_DEPTH_F32 : -1;
    orbhip_ctx *ctx = mpORBextractorLeft ? mpORBextractorLeft->Context() : nullptr;   // (for the error text only)
    const int rc = orbhip_rgbd_depth(ctx, reinterpret_cast<const orbhip_keypoint *>(mvKeys.data()),
                                     reinterpret_cast<const orbhip_keypoint *>(mvKeysUn.data()), N, imDepthRaw.data, type,
                                     imDepthRaw.cols, imDepthRaw.rows, (int)imDepthRaw.step, depthMapFactor, mbf, mvuRight.data(),
                                     mvDepth.data());
    if (rc != ORBHIP_OK)
    {
        hipdetail::Fail("Frame::ComputeStereoFromRGBD", orbhip_last_error(ctx));
        mvuRight.assign(N, -1.0f);
        mvDepth.assign(N, -1.0f);
    }
}

}  // namespace ORB_SLAM2
