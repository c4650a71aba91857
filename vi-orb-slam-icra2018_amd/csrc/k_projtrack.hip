// k_projtrack.hip -- the projection loops of Tracking's two other guided searches on the resident map:
//   k_project_last_frame        ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), ref: src/ORBmatcher.cc:1366-1413
//   k_project_keyframe_points   ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), ref: :1516-1558
// One lane per source feature, blockIdx.y = the frame of a batch.  A lane gathers its point from the store's structure of arrays
// by slot (whole dwordx4 loads), projects it with the arithmetic of host/ORBmatcher.cc's FrameCamera::project (project_point
// below; the shared steps are project_dev.h's) and writes the query of the window search (k_guided.hip), which reads the point's
// descriptor from the store by slot.  Inactive queries are all zero.  The camera record is indexed by blockIdx.y alone, so it
// arrives through scalar loads.
// Divergences from the reference, by design (the reference reaches undefined behaviour there): a point with a non-finite
// position, a non-finite reciprocal depth (z == 0), u or v, dist3D == 0 or non-finite, a non-finite mfMaxDistance / dist3D, or a
// slot that is not live is inactive; so is a source keypoint whose octave is outside [0, nlevels).
#include "project_dev.h"

// The frame searches' pinhole: the reciprocal depth is a DOUBLE division rounded to float (not the float division of isInFrustum
// and Fuse), u = (fx * xc) * invz + cx, closed bounds.  false: outside the image or outside the contract.  *px is what the
// reference's loop has at that point.
__device__ __forceinline__ bool project_point(const orbhip_local_camera &C, const float4 A, ProjPixel *px)
{
    if (!finite3(A.x, A.y, A.z)) return false;
    const float3 Pc = camera_point(C.Rcw, C.tcw, A.x, A.y, A.z);
    const float invz = (float)__ddiv_rn(1.0, (double)Pc.z);                        // ref: :1381, :1530
    if (!isfinite(invz)) return false;
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(C.fx, Pc.x), invz), C.cx);       // :1386-1387, :1532-1533
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(C.fy, Pc.y), invz), C.cy);
    if (!isfinite(u) || !isfinite(v)) return false;
    if (u < C.min_x || u > C.max_x) return false;                                  // :1389-1392, :1535-1538
    if (v < C.min_y || v > C.max_y) return false;
    px->u = u, px->v = v, px->invz = invz;
    return true;
}

__global__ __launch_bounds__(256) void k_project_last_frame(const float4 *__restrict__ geoA, const uint32_t *__restrict__ mflags,
                                                            int maxPoints, const orbhip_local_camera *__restrict__ cams,
                                                            const int32_t *__restrict__ slots,
                                                            const orbhip_keypoint *__restrict__ lastKps,
                                                            const int32_t *__restrict__ motion, const int32_t *__restrict__ nq,
                                                            int capQ, orbhip_proj_query *__restrict__ queries,
                                                            int32_t *__restrict__ nActive)
{
    const int b = blockIdx.y, iq = blockIdx.x * 256 + threadIdx.x;
    const int NQ = min(nq[b], capQ);
    bool active = false;
    if (iq < NQ) {
        const orbhip_local_camera &C = cams[b];
        const size_t at = (size_t)b * capQ + iq;
        orbhip_proj_query q = empty_query();
        const int s = slots[at];                             // -1: no point, an outlier (ref: :1370-1372), a key the store does not know
        uint32_t fl = 0;
        if (s >= 0 && s < maxPoints) fl = mflags[s];
        if (fl & MP_LIVE) {                                  // (the reference does not test isBad() here)
            ProjPixel px;
            const int octave = lastKps[at].octave;           // :1400
            const int nl = min(C.nlevels, 16);
            if (project_point(C, geoA[s], &px) && !(px.invz < 0.0f) && octave >= 0 && octave < nl) {   // :1383
                const int mo = motion[b];
                q.u = px.u;
                q.v = px.v;
                q.radius = __fmul_rn(C.th, C.scale_factors[octave]);                       // :1403
                q.proj_xr = __fsub_rn(px.u, __fmul_rn(C.mbf, px.invz));                    // :1435
                q.min_level = mo == 1 ? octave : mo == 2 ? 0 : octave - 1;                 // :1407-1412
                q.max_level = mo == 1 ? -1 : mo == 2 ? octave : octave + 1;
                q.angle = lastKps[at].angle;                                               // :1461
                q.flags = ORBHIP_Q_ACTIVE | ((fl & ORBHIP_MP_OBSERVED) ? ORBHIP_Q_OBSERVED : 0);
                active = true;
            }
        }
        queries[at] = q;
    }
    count_active(active, nActive + b);
}

// rowIdx[b] = the key frame's row of the table; kfKps [B][capQ] its resident keypoints; slotsOut [B][capQ] = what each entry
// resolves to (-1: nothing), the qslot array of the window search
__global__ __launch_bounds__(256) void k_project_keyframe_points(const float4 *__restrict__ geoA, const float4 *__restrict__ geoB,
                                                                 const uint32_t *__restrict__ mflags, int maxPoints,
                                                                 const uint32_t *__restrict__ marks, const int2 *__restrict__ rows,
                                                                 int nrows, int stride, int maxRow,
                                                                 const int32_t *__restrict__ rowIdx,
                                                                 const orbhip_local_camera *__restrict__ cams,
                                                                 const orbhip_keypoint *__restrict__ kfKps,
                                                                 const int32_t *__restrict__ nq, int capQ,
                                                                 orbhip_proj_query *__restrict__ queries,
                                                                 int32_t *__restrict__ slotsOut, int32_t *__restrict__ nActive)
{
    const int b = blockIdx.y, iq = blockIdx.x * 256 + threadIdx.x;
    const int r = rowIdx[b];
    int NQ = 0;
    const int2 *row = rows;
    if (r >= 0 && r < nrows) {
        row = rows + (size_t)r * stride;
        NQ = min(min(nq[b], capQ), min(row[0].x, maxRow));
    }
    bool active = false;
    if (iq < min(nq[b], capQ)) {
        const orbhip_local_camera &C = cams[b];
        const size_t at = (size_t)b * capQ + iq;
        orbhip_proj_query q = empty_query();
        int s = -1;
        if (iq < NQ) s = kf_entry_slot(row[1 + iq], mflags, maxPoints);    // live, not bad, the entry's generation (:1520-1522)
        if (s >= 0 && marks[s] == 0u) {                                    // sAlreadyFound (:1522)
            const float4 A = geoA[s], N = geoB[s];                         // {P, mfMinDistance}, {normal, mfMaxDistance}
            ProjPixel px;
            do {
                if (!project_point(C, A, &px)) break;                      // (no depth-sign test here, as in the reference)
                const float ox = __fsub_rn(A.x, C.Ow[0]), oy = __fsub_rn(A.y, C.Ow[1]), oz = __fsub_rn(A.z, C.Ow[2]);   // :1541
                const float dist = (float)cv_norm3(ox, oy, oz);            // :1542
                if (!in_distance_window(dist, A.w, N.w)) break;            // :1548-1549
                int level;
                if (!predict_scale(C, N.w, dist, level)) break;            // :1553
                q.u = px.u;
                q.v = px.v;
                q.radius = __fmul_rn(C.th, C.scale_factors[level]);        // :1555
                q.min_level = level - 1;                                   // :1557
                q.max_level = level + 1;
                q.angle = kfKps[at].angle;                                 // :1587
                q.flags = ORBHIP_Q_ACTIVE | ORBHIP_Q_OBSERVED;             // (every feature with a point is closed: `occupied`)
                active = true;
            } while (0);
        }
        queries[at] = q;
        slotsOut[at] = s;
    }
    count_active(active, nActive + b);
}

// nActive[B] must be zero when the kernels start
void launch_project_last_frame(hipStream_t s, const void *geoA, const uint32_t *mflags, int maxPoints, const orbhip_local_camera *cams,
                               const int32_t *slots, const orbhip_keypoint *lastKps, const int32_t *motion, const int32_t *nq, int capQ,
                               int B, orbhip_proj_query *queries, int32_t *nActive)
{
    hipLaunchKernelGGL(k_project_last_frame, dim3((capQ + 255) / 256, B, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA, mflags,
                       maxPoints, cams, slots, lastKps, motion, nq, capQ, queries, nActive);
}

void launch_project_keyframe_points(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints,
                                    const uint32_t *marks, const void *rows, int nrows, int stride, int maxRow, const int32_t *rowIdx,
                                    const orbhip_local_camera *cams, const orbhip_keypoint *kfKps, const int32_t *nq, int capQ, int B,
                                    orbhip_proj_query *queries, int32_t *slotsOut, int32_t *nActive)
{
    hipLaunchKernelGGL(k_project_keyframe_points, dim3((capQ + 255) / 256, B, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, maxPoints, marks, (const int2 *)rows, nrows, stride, maxRow, rowIdx, cams, kfKps,
                       nq, capQ, queries, slotsOut, nActive);
}
