// k_correct.hip -- map points of the resident store moved in place.
//   k_map_correct_sim3  the point loop of LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-568).  Sixteen lanes per point, four
//                       points per wave, as k_map_refresh.  Every lane of a point's row maps the position through Siw and
//                       corrected_Swi itself: the sixteen lanes of a row issue together, so the redundant copies cost no cycle a
//                       lane-0 copy would not, and they save the six shuffles that would carry three doubles to the other lanes;
//                       the transform is one address for the row, so its loads coalesce to one.  The lanes then form their
//                       observers' directions, with the centre the observer has at this point's turn of the reference's sequence
//                       (after its SetPose when 0 <= rank < corr, before it otherwise), and normal_and_depth (refresh_dev.h) does
//                       the rest as for k_map_refresh.  Lane 0 writes geoA and geoB; flag word, generation and descriptor are not
//                       touched.  A slot occurs once per call and a point reads no position but its own, so writing inside the
//                       launch is safe.
//   k_map_correct_se3   the point loop of LoopClosing::RunGlobalBundleAdjustment (ref: :762-797), one thread per point: two gemms
//                       (gemm_row, localmap_dev.h) or the given position.  geoA.xyz alone is written.
// Every double operation of g2o::Sim3::map is individually rounded (docs/parity.md, "CorrectLoop").
#include "refresh_dev.h"

// g2o::Sim3::map (ref: Thirdparty/g2o/g2o/types/sim3.h:144): s*(r*xyz)+t, r*xyz as Eigen 3's Quaternion::_transformVector --
// uv = q.vec x v; uv += uv; v + w*uv + q.vec x uv.  A cross component is a*b - c*d with both products rounded.
__device__ __forceinline__ double cross_term(double a, double b, double c, double d) { return __dsub_rn(__dmul_rn(a, b), __dmul_rn(c, d)); }

__device__ __forceinline__ void sim3_map(const orbhip_sim3d &S, double &x, double &y, double &z)
{
    const double qx = S.q[0], qy = S.q[1], qz = S.q[2], qw = S.q[3];
    double ux = cross_term(qy, z, qz, y), uy = cross_term(qz, x, qx, z), uz = cross_term(qx, y, qy, x);
    ux = __dadd_rn(ux, ux), uy = __dadd_rn(uy, uy), uz = __dadd_rn(uz, uz);
    const double rx = __dadd_rn(__dadd_rn(x, __dmul_rn(qw, ux)), cross_term(qy, uz, qz, uy));
    const double ry = __dadd_rn(__dadd_rn(y, __dmul_rn(qw, uy)), cross_term(qz, ux, qx, uz));
    const double rz = __dadd_rn(__dadd_rn(z, __dmul_rn(qw, uz)), cross_term(qx, uy, qy, ux));
    x = __dadd_rn(__dmul_rn(S.s, rx), S.t[0]);
    y = __dadd_rn(__dmul_rn(S.s, ry), S.t[1]);
    z = __dadd_rn(__dmul_rn(S.s, rz), S.t[2]);
}

__global__ __launch_bounds__(256) void k_map_correct_sim3(const orbhip_correct_xf *__restrict__ xf, const orbhip_correct_kf *__restrict__ kfs,
                                                          const orbhip_refresh_params *__restrict__ prm, const int32_t *__restrict__ slots,
                                                          const int32_t *__restrict__ corr, const int32_t *__restrict__ off,
                                                          const int32_t *__restrict__ obs, const int32_t *__restrict__ refPos,
                                                          const uint8_t *__restrict__ refLevel, int P, int K, int maxPoints, float4 *geoA,
                                                          float4 *geoB, const uint32_t *__restrict__ mflags, uint8_t *__restrict__ status,
                                                          float4 *__restrict__ geoAOut, float4 *__restrict__ geoBOut)
{
    const int p = blockIdx.x * 16 + (threadIdx.x >> 4), lane = threadIdx.x & 15;
    if (p >= P) return;
    const int slot = slots[p];
    if (slot < 0 || slot >= maxPoints) return;   // (the host resolves every key before the launch)
    const int s = off[p], N = off[p + 1] - s;
    const int c = min(max(corr[p], 0), K - 1);
    float4 A = geoA[slot], B = geoB[slot];
    int st = 0;
    if (!(mflags[slot] & ORBHIP_MP_BAD)) {
        double x = (double)A.x, y = (double)A.y, z = (double)A.z;   // Converter::toVector3d
        sim3_map(xf[c].Siw, x, y, z);
        sim3_map(xf[c].corrected_Swi, x, y, z);
        A.x = (float)x, A.y = (float)y, A.z = (float)z;             // Converter::toCvMat: one rounding each
        st = 1;
        if (N > 0) {
            normal_and_depth(A.x, A.y, A.z, N, lane, refPos[p], refLevel[p], prm,
                             [&](int j, float &ox, float &oy, float &oz) {
                                 const orbhip_correct_kf &F = kfs[obs[s + j]];
                                 const float *O = (F.rank >= 0 && F.rank < c) ? F.Ow_after : F.Ow_before;
                                 ox = O[0], oy = O[1], oz = O[2];
                             },
                             B, A.w);
            st = 3;
        }
    }
    if (lane == 0) {
        if (st & 1) geoA[slot] = A;
        if (st & 2) geoB[slot] = B;
        status[p] = (uint8_t)st;
        geoAOut[p] = A;
        geoBOut[p] = B;
    }
}

void launch_map_correct_sim3(hipStream_t s, const orbhip_correct_xf *xf, const orbhip_correct_kf *kfs, const orbhip_refresh_params *prm,
                             const int32_t *slots, const int32_t *corr, const int32_t *off, const int32_t *obs, const int32_t *refPos,
                             const uint8_t *refLevel, int P, int K, int maxPoints, void *geoA, void *geoB, const uint32_t *mflags,
                             uint8_t *status, void *geoAOut, void *geoBOut)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_map_correct_sim3, dim3((P + 15) / 16, 1, 1), dim3(256, 1, 1), 0, s, xf, kfs, prm, slots, corr, off, obs, refPos,
                       refLevel, P, K, maxPoints, (float4 *)geoA, (float4 *)geoB, mflags, status, (float4 *)geoAOut, (float4 *)geoBOut);
}

__global__ __launch_bounds__(256) void k_map_correct_se3(const orbhip_correct_se3 *__restrict__ xf, const int32_t *__restrict__ slots,
                                                         const int32_t *__restrict__ corr, const float *__restrict__ posSet, int P, int K,
                                                         int maxPoints, float4 *geoA, const uint32_t *__restrict__ mflags,
                                                         uint8_t *__restrict__ status, float *__restrict__ posOut)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int slot = slots[p];
    if (slot < 0 || slot >= maxPoints) return;
    const float4 A = geoA[slot];
    float x = A.x, y = A.y, z = A.z;
    int st = 0;
    if (!(mflags[slot] & ORBHIP_MP_BAD)) {
        const int c = corr[p];
        if (c >= 0 && c < K) {
            const orbhip_correct_se3 &T = xf[c];
            const float cx = gemm_row(T.Rcw_before, T.tcw_before[0], x, y, z);       // Xc = Rcw*Xw + tcw
            const float cy = gemm_row(T.Rcw_before + 3, T.tcw_before[1], x, y, z);
            const float cz = gemm_row(T.Rcw_before + 6, T.tcw_before[2], x, y, z);
            x = gemm_row(T.Rwc, T.twc[0], cx, cy, cz);                               // Rwc*Xc + twc
            y = gemm_row(T.Rwc + 3, T.twc[1], cx, cy, cz);
            z = gemm_row(T.Rwc + 6, T.twc[2], cx, cy, cz);
            st = 1;
        } else if (c == -1 && posSet) {
            x = posSet[3 * (size_t)p], y = posSet[3 * (size_t)p + 1], z = posSet[3 * (size_t)p + 2];
            st = 1;
        }
        if (st) {
            float *a = reinterpret_cast<float *>(geoA) + 4 * (size_t)slot;           // geoA.w, mfMinDistance, stays
            a[0] = x, a[1] = y, a[2] = z;
        }
    }
    status[p] = (uint8_t)st;
    posOut[3 * (size_t)p] = x, posOut[3 * (size_t)p + 1] = y, posOut[3 * (size_t)p + 2] = z;
}

void launch_map_correct_se3(hipStream_t s, const orbhip_correct_se3 *xf, const int32_t *slots, const int32_t *corr, const float *posSet,
                            int P, int K, int maxPoints, void *geoA, const uint32_t *mflags, uint8_t *status, float *posOut)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_map_correct_se3, dim3((P + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, xf, slots, corr, posSet, P, K, maxPoints,
                       (float4 *)geoA, mflags, status, posOut);
}
