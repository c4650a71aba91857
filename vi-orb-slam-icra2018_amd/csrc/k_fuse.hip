// k_fuse.hip -- ORBmatcher::Fuse(pKF, vpMapPoints, th) for all the targets of LocalMapping::SearchInNeighbors on the resident map
// (ref: src/ORBmatcher.cc:825-975, src/LocalMapping.cc:2514-2594):
//   k_project_fuse       the projection loop (:842-890).  One lane per (target, source entry), blockIdx.y = the target, whose
//                        camera record therefore arrives through scalar loads.  ROW: the source is a row of the key-frame table
//                        (an entry resolves through kf_entry_slot: live, not bad, the entry's generation); otherwise it is the
//                        slot list an ordered union left on the device, `*nq` long, the same list for every target.  SIM3: the
//                        cameras are decomposed similarities (Fuse(pKF, Scw, ...), ref: :977-1049), proj_xr is 0.  The point is
//                        gathered from the store's structure of arrays by slot (whole dwordx4 loads).  Writes one query per entry
//                        -- all zero when inactive -- and the slot array of the search, and counts the active queries per target.
//   k_fuse_records       the grid-ordered feature records {x, y, octave | index << 8} of all K target sets in one launch
//   k_window_best_sets   the window search of k_window_best_row (k_guided.hip; the same inner loop, window_row_best) with a
//                        per-target record selected by blockIdx.y, the chi-square gate on (Fuse) or off (Fuse with a similarity,
//                        DESIGN.md section 18) and the query's descriptor read from the store by slot.
// The arithmetic of k_project_fuse is that of Fuse, operation for operation, not that of the frame searches (k_projtrack.hip):
// `zc < 0` rejects, the pinhole is fuse_pinhole (project_dev.h, as are the other shared steps), dist3D is cv::norm of P - Ow, and
// the viewing test compares Mat::dot, unrounded, with 0.5 * (double)dist3D.
// Divergences from the reference, by design (it reaches undefined behaviour there): dist3D == 0 or not
// finite, a non-finite mfMaxDistance / dist3D, and an entry that does not resolve are inactive.
#include "project_dev.h"

#include <cstring>

// what k_fuse_records and k_window_best_sets read of target k; indexed by blockIdx.y alone
struct FuseTargetDev {
    const orbhip_keypoint *kps;
    const uint4 *desc;
    const int32_t *cellOff, *cellIdx;
    float4 *rec;                // [n] grid-ordered feature records (scratch of the call)
    const float *uRight;        // [n] or null
    GridParams gp;
    int32_t n, pad;
    float invSigma2[16];
};

template <bool ROW, bool SIM3>
__global__ __launch_bounds__(256) void k_project_fuse(const float4 *__restrict__ geoA, const float4 *__restrict__ geoB,
                                                      const uint32_t *__restrict__ mflags, int maxPoints,
                                                      const uint32_t *__restrict__ marks, const int2 *__restrict__ row, int rowCap,
                                                      const int32_t *__restrict__ slotsIn, const int32_t *__restrict__ nq,
                                                      const uint8_t *__restrict__ skip,
                                                      const orbhip_local_camera *__restrict__ cams, int capQ,
                                                      orbhip_proj_query *__restrict__ queries, int32_t *__restrict__ slotsOut,
                                                      int32_t *__restrict__ nActive)
{
    const int b = blockIdx.y, iq = blockIdx.x * 256 + threadIdx.x;
    const int NQ = ROW ? min(min(row[0].x, rowCap), capQ) : min(nq[0], capQ);
    bool active = false;
    if (iq < capQ) {
        const orbhip_local_camera &C = cams[b];
        const size_t at = (size_t)b * capQ + iq;
        orbhip_proj_query q = empty_query();
        int s = -1;
        if (iq < NQ) {                                                     // !pMP, isBad() (ref: :844-848)
            if (ROW) {
                s = kf_entry_slot(row[1 + iq], mflags, maxPoints);
            } else {
                s = slotsIn[iq];
                if (s < 0 || s >= maxPoints || (mflags[s] & (MP_LIVE | ORBHIP_MP_BAD)) != MP_LIVE) s = -1;
            }
        }
        bool take = s >= 0;
        if (take && skip) take = skip[at] == 0;                            // IsInKeyFrame(pKF) as the caller knows it (:847)
        if (take && marks) take = marks[s] == 0u;                          // IsInKeyFrame(pKF): the target's own row, marked
        if (take) {
            const float4 A = geoA[s], N = geoB[s];                         // {P, mfMinDistance}, {normal, mfMaxDistance}
            ProjPixel px;
            do {
                const float3 Pc = camera_point(C.Rcw, C.tcw, A.x, A.y, A.z);               // :850-851
                if (Pc.z < 0.0f) break;                                                    // :854
                if (!fuse_pinhole(C, C, Pc.x, Pc.y, Pc.z, px)) break;                      // :857-865
                const float ox = __fsub_rn(A.x, C.Ow[0]), oy = __fsub_rn(A.y, C.Ow[1]), oz = __fsub_rn(A.z, C.Ow[2]);   // :872
                const float dist = (float)cv_norm3(ox, oy, oz);                            // :873
                if (!in_distance_window(dist, A.w, N.w)) break;                            // :876
                if (mat_dot3(ox, oy, oz, N.x, N.y, N.z) < __dmul_rn(0.5, (double)dist)) break;   // :882
                int level;
                if (!predict_scale(C, N.w, dist, level)) break;                            // :886
                q.u = px.u;
                q.v = px.v;
                q.radius = __fmul_rn(C.th, C.scale_factors[level]);        // :888
                q.proj_xr = SIM3 ? 0.0f : __fsub_rn(px.u, __fmul_rn(C.mbf, px.invz));      // :868; Fuse(pKF, Scw, ...) has none
                q.min_level = level - 1;                                   // :913
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

__global__ __launch_bounds__(256) void k_fuse_records(const FuseTargetDev *__restrict__ targets)
{
    const FuseTargetDev &T = targets[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= min(T.cellOff[ORBHIP_GRID_CELLS], T.n)) return;
    const int idx = T.cellIdx[j];
    if (idx < 0 || idx >= T.n) return;
    const orbhip_keypoint k = T.kps[idx];
    T.rec[j] = make_float4(k.x, k.y, __int_as_float((k.octave & 255) | (idx << 8)), 0.f);
}

// queries, qslot, bestIdx, bestDist [K][capQ]; an inactive query never reads its slot.  GATE = false: the loop of Fuse(pKF, Scw, ...)
// (ref: src/ORBmatcher.cc:1062-1079), which has no chi-square test; uRight and invSigma2 are not read then.
template <bool GATE>
__global__ __launch_bounds__(256) void k_window_best_sets(const FuseTargetDev *__restrict__ targets,
                                                          const orbhip_proj_query *__restrict__ queries,
                                                          const uint4 *__restrict__ mdesc, const int32_t *__restrict__ qslot, int capQ,
                                                          int32_t *__restrict__ bestIdx, int32_t *__restrict__ bestDist)
{
    __shared__ int s_start[16][16], s_excl[16][17];
    const int b = blockIdx.y, tid = threadIdx.x, gl = tid & 15, row = tid >> 4;
    const int iq = blockIdx.x * 16 + row;
    if (iq >= capQ) return;   // row-uniform
    const FuseTargetDev &T = targets[b];
    const size_t at = (size_t)b * capQ + iq;
    int key = 0x7FFFFFFF, myIdx = -1;
    const orbhip_proj_query q = queries[at];
    int x0, x1, y0, y1;
    if ((q.flags & ORBHIP_Q_ACTIVE) && window_cells(T.gp, q.u, q.v, q.radius, x0, x1, y0, y1)) {
        const uint4 *qd = mdesc + 2 * (size_t)qslot[at];
        const float *sig = T.invSigma2;
        window_row_best(q, x0, x1, y0, y1, qd[0], qd[1], T.desc, T.uRight, T.rec, T.cellOff, GATE,
                        [sig](int oct) { return sig[oct & 15]; }, s_start[row], s_excl[row], gl, key, myIdx);
    }
    window_row_store(key, myIdx, gl, bestIdx + at, bestDist + at);
}

// nActive[K] must be zero when the kernel starts; every query and slot of [K][capQ] is written
void launch_project_fuse_row(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints, const void *row,
                             int rowCap, const uint8_t *skip, const orbhip_local_camera *cams, int capQ, int K,
                             orbhip_proj_query *queries, int32_t *slotsOut, int32_t *nActive)
{
    hipLaunchKernelGGL((k_project_fuse<true, false>), dim3((capQ + 255) / 256, K, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, maxPoints, (const uint32_t *)nullptr, (const int2 *)row, rowCap,
                       (const int32_t *)nullptr, (const int32_t *)nullptr, skip, cams, capQ, queries, slotsOut, nActive);
}

// the source is slots[min(*nq, capQ)] (an ordered union); a slot whose mark word is not zero is inactive
void launch_project_fuse_list(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints,
                              const uint32_t *marks, const int32_t *slots, const int32_t *nq, const orbhip_local_camera *cam, int capQ,
                              orbhip_proj_query *queries, int32_t *slotsOut, int32_t *nActive)
{
    hipLaunchKernelGGL((k_project_fuse<false, false>), dim3((capQ + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, maxPoints, marks, (const int2 *)nullptr, 0, slots, nq, (const uint8_t *)nullptr, cam,
                       capQ, queries, slotsOut, nActive);
}

size_t fuse_target_bytes() { return sizeof(FuseTargetDev); }

void fuse_target_fill(void *dst, const void *kps, const void *desc, const int32_t *cellOff, const int32_t *cellIdx, void *rec,
                      const float *uRight, float minX, float minY, float invW, float invH, int n, const float *invSigma2)
{
    FuseTargetDev t = {};
    t.kps = (const orbhip_keypoint *)kps;
    t.desc = (const uint4 *)desc;
    t.cellOff = cellOff, t.cellIdx = cellIdx;
    t.rec = (float4 *)rec;
    t.uRight = uRight;
    t.gp = {minX, minY, invW, invH};
    t.n = n;
    for (int i = 0; i < 16; i++) t.invSigma2[i] = invSigma2[i];
    memcpy(dst, &t, sizeof t);
}

// the list form for K targets that each carry their own similarity (Fuse(pKF, Scw, ...), ref: :977-1049; SearchByProjection(pKF,
// Scw, ...), :290-360): the same list for every target, skip [K][capQ] or null, marks or null; proj_xr is written as 0
void launch_project_fuse_sim3(hipStream_t s, const void *geoA, const void *geoB, const uint32_t *mflags, int maxPoints,
                              const uint32_t *marks, const int32_t *slots, const int32_t *nq, const uint8_t *skip,
                              const orbhip_local_camera *cams, int capQ, int K, orbhip_proj_query *queries, int32_t *slotsOut,
                              int32_t *nActive)
{
    hipLaunchKernelGGL((k_project_fuse<false, true>), dim3((capQ + 255) / 256, K, 1), dim3(256, 1, 1), 0, s, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, maxPoints, marks, (const int2 *)nullptr, 0, slots, nq, skip, cams, capQ, queries,
                       slotsOut, nActive);
}

// targets [K] (device); maxN = the largest set among them
void launch_window_best_sets(hipStream_t s, const void *targets, int K, int maxN, const orbhip_proj_query *queries, const void *mdesc,
                             const int32_t *qslot, int capQ, int32_t *bestIdx, int32_t *bestDist, bool gate)
{
    hipLaunchKernelGGL(k_fuse_records, dim3((maxN + 255) / 256, K, 1), dim3(256, 1, 1), 0, s, (const FuseTargetDev *)targets);
    const dim3 grid((capQ + 15) / 16, K, 1), block(256, 1, 1);
    if (gate)
        hipLaunchKernelGGL(k_window_best_sets<true>, grid, block, 0, s, (const FuseTargetDev *)targets, queries, (const uint4 *)mdesc, qslot,
                           capQ, bestIdx, bestDist);
    else
        hipLaunchKernelGGL(k_window_best_sets<false>, grid, block, 0, s, (const FuseTargetDev *)targets, queries, (const uint4 *)mdesc, qslot,
                           capQ, bestIdx, bestDist);
}
