// k_sim3search.hip -- ORBmatcher::SearchBySim3 on the resident map (ref: src/ORBmatcher.cc:1102-1326, called at
// src/LoopClosing.cc:375):
//   k_project_sim3   both projection loops (:1148-1192, :1228-1272).  One lane per (direction, row entry), blockIdx.y = the
//                    direction, so the pair record and the three camera records a direction reads (source pose, destination
//                    bounds and scale tables, side 1's intrinsics) arrive through scalar loads.  The body is k_project_fuse's
//                    (k_fuse.hip) with four differences: the camera point is TWO gemms (p = Rsw * Xw + tsw rounded to float, then
//                    sR * p + t); dist3D is cv::norm of that camera point -- there is no P - Ow here; there is no viewing test
//                    and proj_xr is 0; fx, fy, cx, cy are side 1's in BOTH directions (:1105-1108, used at :1170 and :1250),
//                    while the bounds, the scale tables and the grid are the destination's.  Writes one query -- all zero when
//                    inactive -- and one slot per entry of [2][capQ], and counts the active queries per direction.
//   k_sim3_agree     :1221, :1301 and :1310-1323: one lane per feature of key frame 1; th_high on both tables, the mutual naming,
//                    match12, and the count through one ballot and one atomic per wave (count_active).  Every index read from
//                    memory is bounded before it is used.
// The window search between the two is k_window_best_sets<false> (k_fuse.hip) with two target records: direction 0 searches set 2,
// direction 1 set 1.
// Divergences from the reference, by design, as k_project_fuse: dist3D == 0 or not finite, a non-finite mfMaxDistance / dist3D and
// an entry that does not resolve are inactive.
#include "project_dev.h"

#include <cstring>

// what both kernels read of the pair; direction d carries the points of side d + 1 into the other side
struct Sim3PairDev {
    float sR[2][9], t[2][3];   // [0] = sR21, t21 (camera 1 -> camera 2); [1] = sR12, t12
    int32_t row[2], n[2];      // the sides' rows in the key-frame table and their lengths (= their sets' feature counts)
    float th;
    int32_t thHigh;
};

__global__ __launch_bounds__(256) void k_project_sim3(const float4 *__restrict__ geoA, const float4 *__restrict__ geoB,
                                                      const uint32_t *__restrict__ mflags, int maxPoints,
                                                      const int2 *__restrict__ rows, int stride, int maxRow,
                                                      const Sim3PairDev *__restrict__ pair,
                                                      const orbhip_local_camera *__restrict__ cams,
                                                      const uint8_t *__restrict__ taken1, const uint8_t *__restrict__ taken2, int capQ,
                                                      orbhip_proj_query *__restrict__ queries, int32_t *__restrict__ slotsOut,
                                                      int32_t *__restrict__ nActive)
{
    const int b = blockIdx.y, iq = blockIdx.x * 256 + threadIdx.x;
    const Sim3PairDev &P = *pair;
    const orbhip_local_camera &S = cams[b], &D = cams[1 - b], &K1 = cams[0];
    const int r = P.row[b];
    const int2 *row = rows + (size_t)max(r, 0) * stride;
    const int NQ = r < 0 ? 0 : min(min(row[0].x, maxRow), min(P.n[b], capQ));
    const uint8_t *taken = b == 0 ? taken1 : taken2;
    bool active = false;
    if (iq < capQ) {
        const size_t at = (size_t)b * capQ + iq;
        orbhip_proj_query q = empty_query();
        int s = -1;
        if (iq < NQ) s = kf_entry_slot(row[1 + iq], mflags, maxPoints);    // !pMP, isBad() (ref: :1152-1156)
        bool take = s >= 0;
        if (take && taken) take = taken[iq] == 0;                          // vbAlreadyMatched (:1152, :1232)
        if (take) {
            const float4 A = geoA[s], N = geoB[s];                         // {P, mfMinDistance}, {normal, mfMaxDistance}
            ProjPixel px;
            do {
                const float3 P1 = camera_point(S.Rcw, S.tcw, A.x, A.y, A.z);               // :1159 / :1239
                const float3 Pc = camera_point(P.sR[b], P.t[b], P1.x, P1.y, P1.z);         // :1160 / :1240
                if (Pc.z < 0.0f) break;                                                    // :1163
                if (!fuse_pinhole(K1, D, Pc.x, Pc.y, Pc.z, px)) break;     // :1166-1174: key frame 1's intrinsics, both ways
                const float dist = (float)cv_norm3(Pc.x, Pc.y, Pc.z);      // :1179: of the camera point
                if (!in_distance_window(dist, A.w, N.w)) break;            // :1182
                int level;
                if (!predict_scale(D, N.w, dist, level)) break;            // :1186
                q.u = px.u;
                q.v = px.v;
                q.radius = __fmul_rn(P.th, D.scale_factors[level]);        // :1189
                q.min_level = level - 1;                                   // :1207
                q.max_level = level;
                q.flags = ORBHIP_Q_ACTIVE | ORBHIP_Q_OBSERVED;
                active = true;
            } while (0);
        }
        queries[at] = q;
        slotsOut[at] = s;
    }
    count_active(active, nActive + b);
}

// bestIdx, bestDist [2][capQ]; match12 [n1]; *nfound must be zero when the kernel starts
__global__ __launch_bounds__(256) void k_sim3_agree(const Sim3PairDev *__restrict__ pair, const int32_t *__restrict__ bestIdx,
                                                    const int32_t *__restrict__ bestDist, int capQ, int32_t *__restrict__ match12,
                                                    int32_t *__restrict__ nfound)
{
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    const int n1 = min(pair->n[0], capQ), n2 = min(pair->n[1], capQ), thHigh = pair->thHigh;
    bool agreed = false;
    if (i1 < n1) {
        int i2 = bestDist[i1] <= thHigh ? bestIdx[i1] : -1;                // :1221
        if (i2 >= 0 && i2 < n2) {
            const int back = bestDist[capQ + i2] <= thHigh ? bestIdx[capQ + i2] : -1;   // :1301
            agreed = back == i1;                                           // :1316-1317
        }
        match12[i1] = agreed ? i2 : -1;
    }
    count_active(agreed, nfound);
}

size_t sim3_pair_bytes() { return sizeof(Sim3PairDev); }

void sim3_pair_fill(void *dst, const float *sR21, const float *t21, const float *sR12, const float *t12, int row1, int row2, int n1,
                    int n2, float th, int thHigh)
{
    Sim3PairDev p = {};
    for (int k = 0; k < 9; k++) p.sR[0][k] = sR21[k], p.sR[1][k] = sR12[k];
    for (int k = 0; k < 3; k++) p.t[0][k] = t21[k], p.t[1][k] = t12[k];
    p.row[0] = row1, p.row[1] = row2;
    p.n[0] = n1, p.n[1] = n2;
    p.th = th;
    p.thHigh = thHigh;
    memcpy(dst, &p, sizeof p);
}

// cams [2] (device, prepared): side 1, side 2; taken1 [n1] / taken2 [n2] or null; queries, slotsOut [2][capQ] are written whole;
// nActive [2] must be zero when the kernel starts
void launch_project_sim3(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints, const void *rows,
                         int stride, int maxRow, const void *pair, const orbhip_local_camera *cams, const uint8_t *taken1,
                         const uint8_t *taken2, int capQ, orbhip_proj_query *queries, int32_t *slotsOut, int32_t *nActive)
{
    hipLaunchKernelGGL(k_project_sim3, dim3((capQ + 255) / 256, 2, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA, (const float4 *)geoB,
                       mflags, maxPoints, (const int2 *)rows, stride, maxRow, (const Sim3PairDev *)pair, cams, taken1, taken2, capQ, queries,
                       slotsOut, nActive);
}

void launch_sim3_agree(hipStream_t s, const void *pair, const int32_t *bestIdx, const int32_t *bestDist, int capQ, int n1,
                       int32_t *match12, int32_t *nfound)
{
    if (n1 <= 0) return;
    hipLaunchKernelGGL(k_sim3_agree, dim3((n1 + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, (const Sim3PairDev *)pair, bestIdx, bestDist, capQ,
                       match12, nfound);
}
