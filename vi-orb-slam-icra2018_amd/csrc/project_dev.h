// project_dev.h -- the steps that the projection kernels of the guided searches share (k_local_frustum of k_localmap.hip,
// k_project_last_frame and k_project_keyframe_points of k_projtrack.hip, k_project_fuse of k_fuse.hip, k_project_sim3 of
// k_sim3search.hip), and through refresh_dev.h k_map_refresh and k_map_correct_sim3: the one definition of each rule that
// docs/parity.md declares bit-exact.  Every cv::Mat expression as OpenCV 2.4 evaluates it -- the gemm in double with one rounding per
// component, cv::norm and Mat::dot summed in double -- everything else individually rounded float operations.
// What differs between the searches -- which depth-sign test, a float or a double reciprocal, (fx * xc) * invz or fx * (xc * invz),
// closed or half-open bounds, whether there is a viewing test, what dist3D is the norm of -- stays in the kernels (DESIGN.md
// section 26).  Device code only.
#ifndef ORBHIP_PROJECT_DEV_H
#define ORBHIP_PROJECT_DEV_H
#include "localmap_dev.h"

// Xc = R * X + t (ref: src/Frame.cc:621, src/ORBmatcher.cc:850-851, :1159-1160, :1379, :1527): one gemm, each component summed in
// double and rounded to float once (gemm_row)
__device__ __forceinline__ float3 camera_point(const float *__restrict__ R, const float *__restrict__ t, float x, float y, float z)
{
    return make_float3(gemm_row(R, t[0], x, y, z), gemm_row(R + 3, t[1], x, y, z), gemm_row(R + 6, t[2], x, y, z));
}

// cv::norm(NORM_L2) of a CV_32F 3-vector: squares summed in double, the root in double; the caller rounds.  OpenCV sums from 0.0;
// a square is never -0.0, so starting from x * x gives the same bits
__device__ __forceinline__ double cv_norm3(float x, float y, float z)
{
    double sq = __dadd_rn(__dmul_rn((double)x, (double)x), __dmul_rn((double)y, (double)y));
    sq = __dadd_rn(sq, __dmul_rn((double)z, (double)z));
    return __dsqrt_rn(sq);
}

// Mat::dot of two CV_32F 3-vectors: products summed in double FROM 0.0.  The 0.0 is not redundant here: three -0.0 products sum to
// -0.0 without it and to +0.0 with it, and view_cos = dot / dist is an output of orbhip_search_local_points
__device__ __forceinline__ double mat_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    double s = __dadd_rn(0.0, __dmul_rn((double)ax, (double)bx));
    s = __dadd_rn(s, __dmul_rn((double)ay, (double)by));
    return __dadd_rn(s, __dmul_rn((double)az, (double)bz));
}

// dist inside [GetMinDistanceInvariance(), GetMaxDistanceInvariance()] = [0.8f * mfMinDistance, 1.2f * mfMaxDistance] (ref:
// src/MapPoint.cc:388-398; src/Frame.cc:646, src/ORBmatcher.cc:876, :1182, :1548).  dist == 0 or not finite is outside the contract
// (the reference goes on to an undefined int(ceil(inf))): not in the window
__device__ __forceinline__ bool in_distance_window(float dist, float minDistance, float maxDistance)
{
    if (!(dist > 0.0f) || !isfinite(dist)) return false;
    return !(dist < __fmul_rn(0.8f, minDistance) || dist > __fmul_rn(1.2f, maxDistance));
}

// MapPoint::PredictScale (ref: src/MapPoint.cc:417-432): ceil(logf(mfMaxDistance / dist) / mfLogScaleFactor), clamped to
// [0, nlevels - 1], as a count over the camera's host-built threshold table (api_localmap.hip) instead of a device logf.  false: the
// ratio is not finite, which is outside the contract.  (A record that orbhip_local_camera_prepare would refuse must not read past the
// arrays: 16 levels at the most.)
__device__ __forceinline__ bool predict_scale(const orbhip_local_camera &C, float maxDistance, float dist, int &level)
{
    const float ratio = __fdiv_rn(maxDistance, dist);
    if (!isfinite(ratio)) return false;
    level = 0;
    const int nl = min(C.nlevels, 16);
    for (int k = 0; k < nl - 1; k++) level += ratio >= C.level_ratio[k] ? 1 : 0;
    return true;
}

struct ProjPixel {
    float u, v, invz;
};

// The pinhole of Fuse and SearchBySim3 (ref: src/ORBmatcher.cc:857-865, :1166-1174): invz = 1 / z is a FLOAT division (the host
// path's kf_window divides in double and rounds: the two agree for every float, docs/parity.md); x = xc * invz and then
// u = fx * x + cx, each operation rounded on its own; then KeyFrame::IsInImage, with the maximum OUTSIDE and NaN failing.  K = the
// camera whose intrinsics are used, B = the one whose bounds are (SearchBySim3: side 1's and the destination's).  z == 0 and
// non-finite positions need no rule of their own: u or v is then infinite or NaN and fails IsInImage, as in the reference.
__device__ __forceinline__ bool fuse_pinhole(const orbhip_local_camera &K, const orbhip_local_camera &B, float xc, float yc, float zc,
                                             ProjPixel &px)
{
    px.invz = __fdiv_rn(1.0f, zc);
    const float x = __fmul_rn(xc, px.invz), y = __fmul_rn(yc, px.invz);
    px.u = __fadd_rn(__fmul_rn(K.fx, x), K.cx);
    px.v = __fadd_rn(__fmul_rn(K.fy, y), K.cy);
    return px.u >= B.min_x && px.u < B.max_x && px.v >= B.min_y && px.v < B.max_y;
}

// the query of a point that does not take part: all zero
__device__ __forceinline__ orbhip_proj_query empty_query() { return {0.f, 0.f, 0.f, 0.f, 0, 0, 0.f, 0}; }

#endif
