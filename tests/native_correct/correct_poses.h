// correct_poses.h -- what test_correct.cpp and tools/native/correct_latency.cpp share: the programs' random numbers, and the Sim3
// algebra that stays with the caller of LocalMapSearch::CorrectLoopPoints (the composition of poses, inverse(), the SE3 a corrected
// Sim3 becomes), in plain double arithmetic.
#ifndef ORBHIP_TESTS_CORRECT_POSES_H
#define ORBHIP_TESTS_CORRECT_POSES_H
#include <cmath>
#include <cstring>

#include "LocalMap.h"

using namespace ORB_SLAM2;
typedef LocalMapSearch::Sim3d Sim3d;
typedef LocalMapSearch::LoopCorrection LoopCorrection;

static unsigned g_seed = 1;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) % n; }
static double drand(double lo, double hi) { return lo + (hi - lo) * (double)rnd(1 << 16) / 65536.0; }

struct Pose { double q[4], t[3], s; };

// ---- the caller's Sim3 algebra, in plain double arithmetic ----
static void qmul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
static void qnormalise(double q[4])
{
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= n;
}
static void rotation(const double q[4], double R[9])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    memcpy(R, r, sizeof r);
}
static Pose random_pose()
{
    Pose p;
    for (int i = 0; i < 4; i++) p.q[i] = drand(-1, 1);
    qnormalise(p.q);
    for (int i = 0; i < 3; i++) p.t[i] = drand(-3, 3);
    p.s = 1.0;
    return p;
}
// a nearby pose: a small turn, a small shift, and the scale given
static Pose nudged(const Pose &p, double scale)
{
    Pose o;
    double dq[4] = {drand(-0.02, 0.02), drand(-0.02, 0.02), drand(-0.02, 0.02), 1.0};
    qnormalise(dq);
    qmul(dq, p.q, o.q);
    qnormalise(o.q);
    for (int i = 0; i < 3; i++) o.t[i] = p.t[i] + drand(-0.2, 0.2);
    o.s = scale;
    return o;
}
static Sim3d as_sim3(const Pose &p)
{
    Sim3d S;
    memcpy(S.q, p.q, sizeof S.q), memcpy(S.t, p.t, sizeof S.t);
    S.s = p.s;
    return S;
}
static Sim3d inverse(const Pose &p)   // g2o::Sim3::inverse(): (conj(r), -(1/s) conj(r)*t, 1/s)
{
    Sim3d S;
    double R[9];
    S.q[0] = -p.q[0], S.q[1] = -p.q[1], S.q[2] = -p.q[2], S.q[3] = p.q[3];
    rotation(S.q, R);
    for (int r = 0; r < 3; r++) S.t[r] = -(R[3 * r] * p.t[0] + R[3 * r + 1] * p.t[1] + R[3 * r + 2] * p.t[2]) / p.s;
    S.s = 1.0 / p.s;
    return S;
}
static cv::Mat as_se3(const Pose &p)   // Converter::toCvSE3(R, t / s)
{
    double R[9];
    rotation(p.q, R);
    cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T.at<float>(r, c) = (float)R[3 * r + c];
        T.at<float>(r, 3) = (float)(p.t[r] * (1. / p.s));
    }
    T.at<float>(3, 3) = 1.f;
    return T;
}

#endif
