// rgbd_depth.h -- Frame::ComputeStereoFromRGBD for ONE keypoint (ref: src/Frame.cc:987-1008) with the
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) in front of it (ref: src/Tracking.cc:924-925) folded into the read: the
// converted map is never materialised, the one pixel the keypoint looks at is converted as cvtScale_<T, float, float> with
// beta = 0 converts it.  Shared by k_rgbd_depth (k_ingest.hip) and the host gather of the single-frame calls
// (api_ingest.hip): three individually rounded float operations -- a multiply, a divide, a subtract -- with no contraction
// (__f*_rn on the device, -ffp-contract=off on the host), so both sides agree bit for bit.
#ifndef ORB_RGBD_DEPTH_H
#define ORB_RGBD_DEPTH_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/orbhip.h"

#if defined(__HIPCC__)
#define ORB_RGBD_FN __host__ __device__ __forceinline__
#else
#define ORB_RGBD_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define ORB_FMUL(a, b) __fmul_rn((a), (b))
#define ORB_FDIV(a, b) __fdiv_rn((a), (b))
#define ORB_FSUB(a, b) __fsub_rn((a), (b))
#else
// host: compile with -ffp-contract=off
#define ORB_FMUL(a, b) ((a) * (b))
#define ORB_FDIV(a, b) ((a) / (b))
#define ORB_FSUB(a, b) ((a) - (b))
#endif

// does a map of this type and factor go through convertTo at all?  (ref: src/Tracking.cc:924)
ORB_RGBD_FN bool orb_rgbd_scales(int depth_type, float factor)
{
    return depth_type != ORBHIP_DEPTH_F32 || fabsf(ORB_FSUB(factor, 1.0f)) > 1e-5f;
}

// (x, y): the DISTORTED keypoint, truncated as Mat::at<float>(float, float) truncates its arguments; x_un: the undistorted one.
// `map`: one frame's depth map, rows `stride` bytes apart.  A keypoint outside the map has no depth (the reference reads out of
// bounds there); so has a NaN, which fails d > 0 as in the reference.
ORB_RGBD_FN void orb_rgbd_depth_one(float x, float y, float x_un, const void *map, int depth_type, int dw, int dh, size_t stride,
                                    float factor, bool scales, float mbf, float *u_right, float *depth)
{
    float d = -1.0f;
    // -1 < x < dw is 0 <= (int)x < dw, and no NaN or huge value reaches the conversion
    if (x > -1.0f && x < (float)dw && y > -1.0f && y < (float)dh) {
        const int u = (int)x, v = (int)y;
        const uint8_t *row = (const uint8_t *)map + (size_t)v * stride;
        if (depth_type == ORBHIP_DEPTH_U16) {
            uint16_t raw;
            memcpy(&raw, row + (size_t)u * 2, 2);
            d = ORB_FMUL((float)raw, factor);
        } else {
            memcpy(&d, row + (size_t)u * 4, 4);
            if (scales) d = ORB_FMUL(d, factor);
        }
    }
    if (d > 0.0f) {
        *depth = d;
        *u_right = ORB_FSUB(x_un, ORB_FDIV(mbf, d));
    } else {
        *depth = -1.0f;
        *u_right = -1.0f;
    }
}

#endif
