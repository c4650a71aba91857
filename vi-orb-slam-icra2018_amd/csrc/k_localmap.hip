// k_localmap.hip -- the resident map-point store and the frustum test of Tracking::SearchLocalPoints
// (ref: src/Tracking.cc:2315-2365, src/Frame.cc:613-669 isInFrustum, src/MapPoint.cc:388-432, src/ORBmatcher.cc:45-137).
//   k_map_scatter     batched upsert: staged records -> the store's slots (structure of arrays: two 16-byte geometry
//                     records, a flag word and the 32-byte descriptor per slot, each in an array of its own, so that the
//                     gather below is made of whole dwordx4 loads);
//   k_map_flags       flag words alone (observation counts and bad flags change far more often than geometry);
//   k_local_frustum   one lane per local point: gathers its slot, evaluates isInFrustum in the reference's order with the
//                     reference's roundings, writes the record the reference leaves in the MapPoint and the query of the
//                     window search (k_guided.hip), which reads the point's descriptor from the store by slot.
// isInFrustum's own choices between the shared steps (project_dev.h): `PcZ < 0` rejects, invz is a FLOAT division,
// u = (fx * PcX) * invz + cx, the bounds are closed, and the viewing test compares the rounded cosine with the camera's limit.
#include "project_dev.h"

__global__ __launch_bounds__(256) void k_map_scatter(const int32_t *__restrict__ slot, const float4 *__restrict__ a,
                                                     const float4 *__restrict__ b, const uint32_t *__restrict__ flags,
                                                     const uint4 *__restrict__ desc, int n, int maxPoints,
                                                     float4 *__restrict__ geoA, float4 *__restrict__ geoB,
                                                     uint32_t *__restrict__ mflags, uint4 *__restrict__ mdesc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i];
    if (s < 0 || s >= maxPoints) return;
    geoA[s] = a[i];
    geoB[s] = b[i];
    mflags[s] = flags[i];
    mdesc[2 * (size_t)s] = desc[2 * (size_t)i];
    mdesc[2 * (size_t)s + 1] = desc[2 * (size_t)i + 1];
}

__global__ __launch_bounds__(256) void k_map_flags(const int32_t *__restrict__ slot, const uint32_t *__restrict__ flags, int n,
                                                   int maxPoints, uint32_t *__restrict__ mflags)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i];
    if (s < 0 || s >= maxPoints) return;
    mflags[s] = flags[i];
}

__global__ __launch_bounds__(256) void k_local_frustum(const float4 *__restrict__ geoA, const float4 *__restrict__ geoB,
                                                       const uint32_t *__restrict__ mflags, int maxPoints,
                                                       const orbhip_local_camera *__restrict__ cams,
                                                       const int32_t *__restrict__ slots, const uint8_t *__restrict__ skip,
                                                       const int32_t *__restrict__ nq, int capQ,
                                                       orbhip_local_point *__restrict__ points,
                                                       orbhip_proj_query *__restrict__ queries,
                                                       int32_t *__restrict__ nToMatch)
{
    const int b = blockIdx.y, iq = blockIdx.x * 256 + threadIdx.x;
    const int NQ = min(nq[b], capQ);
    bool inView = false;
    if (iq < NQ) {
        const orbhip_local_camera &C = cams[b];
        const size_t at = (size_t)b * capQ + iq;
        orbhip_local_point rec = {0.f, 0.f, 0.f, 0.f, 0, 0};
        orbhip_proj_query q = empty_query();
        const int s = slots[at];
        uint32_t fl = 0;
        if (s >= 0 && s < maxPoints && !skip[at]) fl = mflags[s];
        if ((fl & MP_LIVE) && !(fl & ORBHIP_MP_BAD)) {
            const float4 A = geoA[s], N = geoB[s];   // {P, mfMinDistance}, {normal, mfMaxDistance}
            do {
                if (!finite3(A.x, A.y, A.z)) break;   // outside the contract: not in view
                const float3 Pc = camera_point(C.Rcw, C.tcw, A.x, A.y, A.z);
                if (Pc.z < 0.0f) break;                                                    // ref: src/Frame.cc:627
                const float invz = __fdiv_rn(1.0f, Pc.z);
                const float u = __fadd_rn(__fmul_rn(__fmul_rn(C.fx, Pc.x), invz), C.cx);   // :632-633
                const float v = __fadd_rn(__fmul_rn(__fmul_rn(C.fy, Pc.y), invz), C.cy);
                if (u < C.min_x || u > C.max_x) break;
                if (v < C.min_y || v > C.max_y) break;
                const float ox = __fsub_rn(A.x, C.Ow[0]), oy = __fsub_rn(A.y, C.Ow[1]), oz = __fsub_rn(A.z, C.Ow[2]);   // :643
                const float dist = (float)cv_norm3(ox, oy, oz);
                if (!in_distance_window(dist, A.w, N.w)) break;                            // :646
                const float viewCos = (float)__ddiv_rn(mat_dot3(ox, oy, oz, N.x, N.y, N.z), (double)dist);   // :652
                if (viewCos < C.viewing_cos_limit) break;
                int level;
                if (!predict_scale(C, N.w, dist, level)) break;
                float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;                           // src/ORBmatcher.cc:131-137
                if (C.th != 1.0f) r = __fmul_rn(r, C.th);                                  // :65-66
                rec.u = u;
                rec.v = v;
                rec.proj_xr = __fsub_rn(u, __fmul_rn(C.mbf, invz));                        // src/Frame.cc:663
                rec.view_cos = viewCos;
                rec.level = level;
                rec.in_view = 1;
                q.u = u;
                q.v = v;
                q.radius = __fmul_rn(r, C.scale_factors[level]);
                q.proj_xr = rec.proj_xr;
                q.min_level = level - 1;
                q.max_level = level;
                q.flags = ORBHIP_Q_ACTIVE | ((fl & ORBHIP_MP_OBSERVED) ? ORBHIP_Q_OBSERVED : 0);
                inView = true;
            } while (0);
        }
        points[at] = rec;
        queries[at] = q;
    }
    count_active(inView, nToMatch + b);
}

void launch_map_scatter(hipStream_t s, const int32_t *slot, const void *a, const void *b, const uint32_t *flags, const void *desc,
                        int n, int maxPoints, void *geoA, void *geoB, uint32_t *mflags, void *mdesc)
{
    hipLaunchKernelGGL(k_map_scatter, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slot, (const float4 *)a, (const float4 *)b,
                       flags, (const uint4 *)desc, n, maxPoints, (float4 *)geoA, (float4 *)geoB, mflags, (uint4 *)mdesc);
}

void launch_map_flags(hipStream_t s, const int32_t *slot, const uint32_t *flags, int n, int maxPoints, uint32_t *mflags)
{
    hipLaunchKernelGGL(k_map_flags, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slot, flags, n, maxPoints, mflags);
}

// nToMatch[B] must be zero when the kernel starts
void launch_local_frustum(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints,
                          const orbhip_local_camera *cams, const int32_t *slots, const uint8_t *skip, const int32_t *nq, int capQ,
                          int B, orbhip_local_point *points, orbhip_proj_query *queries, int32_t *nToMatch)
{
    hipLaunchKernelGGL(k_local_frustum, dim3((capQ + 255) / 256, B, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, maxPoints, cams, slots, skip, nq, capQ, points, queries, nToMatch);
}
