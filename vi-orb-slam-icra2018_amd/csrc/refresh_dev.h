// refresh_dev.h -- MapPoint::UpdateNormalAndDepth (ref: src/MapPoint.cc:345-386) for one point on one 16-lane row, shared by
// k_map_refresh (k_refresh.hip) and k_map_correct_sim3 (k_correct.hip): the one copy of this arithmetic.  The two kernels differ
// in where an observer's camera centre comes from, which the CENTRE functor hides: centre(j, x, y, z) gives the centre of the
// observer at list position j.  Every float / double operation is individually rounded (docs/parity.md, "UpdateNormalAndDepth").
#ifndef ORBHIP_REFRESH_DEV_H
#define ORBHIP_REFRESH_DEV_H
#include "project_dev.h"   // cv_norm3

// The point at (px, py, pz) with N > 0 observers; lane = 0..15 of the row, every lane of the row arrives.  refPos = the position of
// mpRefKF in the list, level = the octave of its feature.  Each lane forms its observers' scaled viewing directions; the running sum
// is added in list order through a shuffle chain (docs/parity.md: order-dependent loops keep their order).  Every lane leaves with
// the same B = {normal, mfMaxDistance} and minDist = mfMinDistance.
template <typename CENTRE>
__device__ __forceinline__ void normal_and_depth(float px, float py, float pz, int N, int lane, int refPos, int level,
                                                 const orbhip_refresh_params *__restrict__ prm, CENTRE centre, float4 &B, float &minDist)
{
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int i0 = 0; i0 < N; i0 += 16) {
        const int i = i0 + lane;
        float tx = 0.f, ty = 0.f, tz = 0.f;
        if (i < N) {
            float ox, oy, oz;
            centre(i, ox, oy, oz);
            const float dx = __fsub_rn(px, ox), dy = __fsub_rn(py, oy), dz = __fsub_rn(pz, oz);
            const float a = (float)__ddiv_rn(1.0, cv_norm3(dx, dy, dz));   // normali / norm: a MatExpr scaled by 1.0 / norm
            tx = __fmul_rn(dx, a), ty = __fmul_rn(dy, a), tz = __fmul_rn(dz, a);
        }
        const int m = min(16, N - i0);
        for (int jj = 0; jj < m; jj++) {   // normal = normal + alpha * normali, in list order
            nx = __fadd_rn(__shfl(tx, jj, 16), nx);
            ny = __fadd_rn(__shfl(ty, jj, 16), ny);
            nz = __fadd_rn(__shfl(tz, jj, 16), nz);
        }
    }
    const float invN = (float)__ddiv_rn(1.0, (double)N);
    float rx, ry, rz;
    centre(min(max(refPos, 0), N - 1), rx, ry, rz);
    const float dist = (float)cv_norm3(__fsub_rn(px, rx), __fsub_rn(py, ry), __fsub_rn(pz, rz));
    const int lv = min(max(level, 0), ORBHIP_MAX_LEVELS - 1);
    const int top = min(max(prm->nlevels - 1, 0), ORBHIP_MAX_LEVELS - 1);
    B.x = __fmul_rn(nx, invN), B.y = __fmul_rn(ny, invN), B.z = __fmul_rn(nz, invN);
    B.w = __fmul_rn(dist, prm->scale_factors[lv]);
    minDist = __fdiv_rn(B.w, prm->scale_factors[top]);
}

#endif
