// k_localmap.hip -- the resident map-point store and the frustum test of Tracking::SearchLocalPoints
// (ref: src/Tracking.cc:2315-2365, src/Frame.cc:613-669 isInFrustum, src/MapPoint.cc:388-432, src/ORBmatcher.cc:45-137).
//   k_map_scatter     batched upsert: staged records -> the store's slots (structure of arrays: two 16-byte geometry
//                     records, a flag word and the 32-byte descriptor per slot, each in an array of its own, so that the
//                     gather below is made of whole dwordx4 loads);
//   k_map_flags       flag words alone (observation counts and bad flags change far more often than geometry);
//   k_local_frustum   one lane per local point: gathers its slot, evaluates isInFrustum in the reference's order with the
//                     reference's roundings, writes the record the reference leaves in the MapPoint and the query of the
//                     window search (k_guided.hip), which reads the point's descriptor from the store by slot.
// The arithmetic: every cv::Mat expression as OpenCV 2.4 evaluates it -- the gemm in double with one
// rounding per component, cv::norm and Mat::dot summed in double -- everything else individually rounded float operations.
// The scale level is a count over a host-built threshold table (api_localmap.hip) instead of a device logf.
#include "localmap_dev.h"

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
        orbhip_proj_query q = {0.f, 0.f, 0.f, 0.f, 0, 0, 0.f, 0};
        const int s = slots[at];
        uint32_t fl = 0;
        if (s >= 0 && s < maxPoints && !skip[at]) fl = mflags[s];
        if ((fl & MP_LIVE) && !(fl & ORBHIP_MP_BAD)) {
            const float4 A = geoA[s], N = geoB[s];   // {P, mfMinDistance}, {normal, mfMaxDistance}
            do {
                if (!finite3(A.x, A.y, A.z)) break;   // outside the contract: not in view
                const float PcX = gemm_row(C.Rcw, C.tcw[0], A.x, A.y, A.z);
                const float PcY = gemm_row(C.Rcw + 3, C.tcw[1], A.x, A.y, A.z);
                const float PcZ = gemm_row(C.Rcw + 6, C.tcw[2], A.x, A.y, A.z);
                if (PcZ < 0.0f) break;                                                     // ref: src/Frame.cc:627
                const float invz = __fdiv_rn(1.0f, PcZ);
                const float u = __fadd_rn(__fmul_rn(__fmul_rn(C.fx, PcX), invz), C.cx);    // :632-633
                const float v = __fadd_rn(__fmul_rn(__fmul_rn(C.fy, PcY), invz), C.cy);
                if (u < C.min_x || u > C.max_x) break;
                if (v < C.min_y || v > C.max_y) break;
                const float ox = __fsub_rn(A.x, C.Ow[0]), oy = __fsub_rn(A.y, C.Ow[1]), oz = __fsub_rn(A.z, C.Ow[2]);   // :643
                double sq = __dadd_rn(0.0, __dmul_rn((double)ox, (double)ox));
                sq = __dadd_rn(sq, __dmul_rn((double)oy, (double)oy));
                sq = __dadd_rn(sq, __dmul_rn((double)oz, (double)oz));
                const float dist = (float)__dsqrt_rn(sq);
                if (!(dist > 0.0f) || !isfinite(dist)) break;                              // outside the contract
                if (dist < __fmul_rn(0.8f, A.w) || dist > __fmul_rn(1.2f, N.w)) break;     // :646, src/MapPoint.cc:388-398
                double dot = __dadd_rn(0.0, __dmul_rn((double)ox, (double)N.x));
                dot = __dadd_rn(dot, __dmul_rn((double)oy, (double)N.y));
                dot = __dadd_rn(dot, __dmul_rn((double)oz, (double)N.z));
                const float viewCos = (float)__ddiv_rn(dot, (double)dist);                 // :652
                if (viewCos < C.viewing_cos_limit) break;
                const float ratio = __fdiv_rn(N.w, dist);                                  // src/MapPoint.cc:417-432
                if (!isfinite(ratio)) break;                                               // outside the contract
                int level = 0;
                const int nl = min(C.nlevels, 16);   // (a record that orbhip_local_camera_prepare would refuse must not read past the arrays)
                for (int k = 0; k < nl - 1; k++) level += ratio >= C.level_ratio[k] ? 1 : 0;
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
    const unsigned long long m = __ballot(inView);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(nToMatch + b, __popcll(m));
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
