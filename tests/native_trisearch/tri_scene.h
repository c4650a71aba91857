// tri_scene.h -- key frames for the TriangulationSearch test programs: K + 1 views of one set of "world" features (descriptor,
// image position, vocabulary node), each view with its own subset, a few flipped descriptor bits, pixel noise, map points on
// part of the features, a pose and an F12 of its own.  Plus SearchForTriangulation (ref: src/ORBmatcher.cc:657-827) restated
// on flat arrays, which the mock of the C entry point and the expectation of the mock test share.
#ifndef ORBHIP_TESTS_TRI_SCENE_H
#define ORBHIP_TESTS_TRI_SCENE_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "slamlite.h"

namespace tri
{
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

struct Rng {
    unsigned long long s;
    explicit Rng(unsigned long long seed) : s(seed * 2654435761ull + 88172645463325252ull) {}
    double u()   // xorshift64*, [0, 1)
    {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return (double)((s * 2685821657736338717ull) >> 11) / 9007199254740992.0;
    }
    int below(int n) { return (int)(u() * n); }
};

struct World {
    int n;
    std::vector<uint8_t> desc;                 // n x 32
    std::vector<float> x, y, angle;
    std::vector<int> node, octave;
    World(int count, Rng &r, int nnodes = 37) : n(count), desc((size_t)count * 32), x(count), y(count), angle(count), node(count), octave(count)
    {
        for (size_t i = 0; i < desc.size(); i++) desc[i] = (uint8_t)r.below(256);
        for (int i = 0; i < n; i++) {
            x[i] = 40.f + (float)r.u() * 560.f;
            y[i] = 20.f + (float)r.below(220) * 2.f;   // rows two pixels apart: several features share an epipolar line
            angle[i] = (float)r.u() * 360.f;
            node[i] = 100 + i % nnodes;
            octave[i] = r.below(4);
        }
    }
};

inline cv::Mat pose(float ay, float tx, float ty, float tz)
{
    cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
    const float c = cosf(ay), s = sinf(ay);
    const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) T.at<float>(r, k) = R[r * 3 + k];
    T.at<float>(0, 3) = tx; T.at<float>(1, 3) = ty; T.at<float>(2, 3) = tz; T.at<float>(3, 3) = 1.f;
    return T;
}

// One view: nfeat features of the world.  stereo 0: mvuRight left empty (a monocular key frame as the drop-in sees it), 1: about
// 60 % of the features have a right coordinate, 2: monocular with mvuRight filled with -1 (as the reference fills it).
inline void make_keyframe(KeyFrame &k, const World &W, Rng &r, int nfeat, int stereo, float shift, const cv::Mat &Tcw,
                          std::deque<MapPoint> &points, bool bow = true)
{
    k.N = nfeat;
    k.mvKeys.assign(nfeat, cv::KeyPoint());
    k.mDescriptors = cv::Mat(nfeat, 32, CV_8U);
    k.mvpMapPoints.assign(nfeat, static_cast<MapPoint *>(NULL));
    k.mFeatVec.clear();
    k.mvuRight.clear();
    for (int i = 0; i < nfeat; i++) {
        const int w = r.below(W.n);
        cv::KeyPoint &kp = k.mvKeys[i];
        kp.pt.x = W.x[w] - shift + (float)(r.u() - 0.5);
        kp.pt.y = W.y[w] + (float)(r.below(3) - 1) * 0.4f;
        kp.octave = W.octave[w];
        kp.angle = fmodf(W.angle[w] + (float)r.u() * 8.f + (r.below(10) == 0 ? 90.f : 0.f), 360.f);
        kp.size = 31.f;
        memcpy(k.mDescriptors.ptr(i), &W.desc[(size_t)w * 32], 32);
        for (int f = r.below(7); f > 0; f--) k.mDescriptors.ptr(i)[r.below(32)] ^= (uint8_t)(1 << r.below(8));
        if (bow) k.mFeatVec.addFeature(W.node[w], i);
        if (r.below(10) < 3) {
            points.push_back(MapPoint());
            k.mvpMapPoints[i] = &points.back();
        }
        if (stereo) k.mvuRight.push_back(stereo == 1 && r.below(10) < 6 ? kp.pt.x - 5.f : -1.f);
    }
    k.mvKeysUn = k.mvKeys;
    k.fx = 458.654f; k.fy = 457.296f; k.cx = 367.215f; k.cy = 248.375f;
    k.mvScaleFactors.assign(8, 1.f);
    k.mvLevelSigma2.assign(8, 1.f);
    for (int l = 1; l < 8; l++) {
        k.mvScaleFactors[l] = k.mvScaleFactors[l - 1] * 1.2f;
        k.mvLevelSigma2[l] = k.mvScaleFactors[l] * k.mvScaleFactors[l];
    }
    k.Tcw = Tcw.clone();
    k.Ow = cv::Mat(3, 1, CV_32F);
    for (int a = 0; a < 3; a++) {   // Ow = -R' t
        double s = 0;
        for (int b = 0; b < 3; b++) s += (double)Tcw.at<float>(b, a) * (double)Tcw.at<float>(b, 3);
        k.Ow.at<float>(a, 0) = (float)-s;
    }
    k.mnMinX = 0; k.mnMinY = 0; k.mnMaxX = 640; k.mnMaxY = 480;
    k.mfGridElementWidthInv = 64.f / 640.f;
    k.mfGridElementHeightInv = 48.f / 480.f;
}

// epipolar lines = image rows, turned a little differently for every neighbour
inline cv::Mat make_F12(int k)
{
    const float e = 1e-6f * (float)(k % 5);
    const float Fv[9] = {e, 4.f * e, -0.0004f * (float)(k % 3), -4.f * e, e, -1.f, 0.0003f * (float)(k % 4), 1.f, 0.01f * (float)(k % 2)};
    cv::Mat F(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) F.at<float>(i / 3, i % 3) = Fv[i];
    return F;
}

struct Scene {
    std::deque<KeyFrame> kf;       // kf[0]: the new key frame; kf[1 ..]: its neighbours
    std::deque<MapPoint> points;
    std::vector<cv::Mat> F12;      // per neighbour
    std::vector<KeyFrame *> nb;
};

// stereoOf(k): the `stereo` argument of make_keyframe for key frame k; sizes differ from key frame to key frame
template <class F>
inline void make_scene(Scene &S, int K, int nfeat, unsigned long long seed, F stereoOf, int nnodes = 37)
{
    Rng r(seed);
    World W(nfeat * 2, r, nnodes);
    S.kf.resize(K + 1);
    for (int k = 0; k <= K; k++) {
        make_keyframe(S.kf[k], W, r, k == 0 ? nfeat : nfeat - 17 * (k % 4) - k, stereoOf(k), k == 0 ? 0.f : 3.f * (float)k,
                      pose(0.01f * (float)k, -0.2f * (float)k, 0.01f * (float)(k % 3), 0.03f + 0.02f * (float)(k % 2)), S.points);
        if (k > 0) {
            S.nb.push_back(&S.kf[k]);
            S.F12.push_back(make_F12(k));
        }
    }
}

// ---- SearchForTriangulation on flat arrays (ref: src/ORBmatcher.cc:657-827, CheckDistEpipolarLine :140-157, ComputeThreeMaxima
// :1629-1670).  kps: {x, y, size, angle, response, octave, class_id} records of 28 bytes; FeatureVectors as CSR over ascending
// node ids.  m12[n1] <- index in key frame 2 or -1; returns the number of matches.
struct Kp {
    float x, y, size, angle, response;
    int octave, class_id;
};
inline int popcount256(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}
inline void three_maxima(const std::vector<int> *histo, int L, int &ind1, int &ind2, int &ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
}
inline int flat_search(const Kp *k1, const uint8_t *d1, int n1, const uint8_t *skip1, const float *ur1, const int32_t *node1,
                       const int32_t *off1, const int32_t *idx1, int ng1, const Kp *k2, const uint8_t *d2, const uint8_t *skip2,
                       const float *ur2, const int32_t *node2, const int32_t *off2, const int32_t *idx2, int ng2, const float F[9],
                       float ex, float ey, const float *sf2, const float *sigma2, bool onlyStereo, bool checkOri, int32_t *m12)
{
    for (int i = 0; i < n1; i++) m12[i] = -1;
    std::vector<int> hist[30];
    int nm = 0;
    for (int g1 = 0, g2 = 0; g1 < ng1 && g2 < ng2;) {
        if (node1[g1] < node2[g2]) { g1++; continue; }
        if (node1[g1] > node2[g2]) { g2++; continue; }
        for (int a = off1[g1]; a < off1[g1 + 1]; a++) {
            const int i1 = idx1[a];
            if (skip1[i1]) continue;
            const bool st1 = ur1 && ur1[i1] >= 0;
            if (onlyStereo && !st1) continue;
            int best = 50, arg = -1;
            for (int b = off2[g2]; b < off2[g2 + 1]; b++) {
                const int i2 = idx2[b];
                if (skip2[i2]) continue;
                const bool st2 = ur2 && ur2[i2] >= 0;
                if (onlyStereo && !st2) continue;
                const int d = popcount256(d1 + (size_t)i1 * 32, d2 + (size_t)i2 * 32);
                if (d > 50 || d > best) continue;
                if (!st1 && !st2) {
                    const float dx = ex - k2[i2].x, dy = ey - k2[i2].y;
                    if (dx * dx + dy * dy < 100 * sf2[k2[i2].octave]) continue;
                }
                const float la = k1[i1].x * F[0] + k1[i1].y * F[3] + F[6];
                const float lb = k1[i1].x * F[1] + k1[i1].y * F[4] + F[7];
                const float lc = k1[i1].x * F[2] + k1[i1].y * F[5] + F[8];
                const float num = la * k2[i2].x + lb * k2[i2].y + lc;
                const float den = la * la + lb * lb;
                if (den == 0) continue;
                const float dsqr = num * num / den;
                if (dsqr < 3.84 * sigma2[k2[i2].octave]) { arg = i2; best = d; }
            }
            if (arg < 0) continue;
            m12[i1] = arg;
            nm++;
            if (checkOri) {
                float rot = k1[i1].angle - k2[arg].angle;
                if (rot < 0.0) rot += 360.0f;
                int bin = (int)roundf(rot * (1.0f / 30));
                if (bin == 30) bin = 0;
                hist[bin].push_back(i1);
            }
        }
        g1++;
        g2++;
    }
    if (checkOri) {
        int a, b, c;
        three_maxima(hist, 30, a, b, c);
        for (int i = 0; i < 30; i++) {
            if (i == a || i == b || i == c) continue;
            for (size_t j = 0; j < hist[i].size(); j++) { m12[hist[i][j]] = -1; nm--; }
        }
    }
    return nm;
}

}  // namespace tri

#endif
