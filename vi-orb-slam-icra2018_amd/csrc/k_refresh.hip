// k_refresh.hip -- MapPoint::ComputeDistinctiveDescriptors (ref: src/MapPoint.cc:257-322) and MapPoint::UpdateNormalAndDepth
// (ref: :345-386) for a batch of points of the resident store, in place.
//   k_map_refresh   sixteen lanes per point, four points per wave, as k_distinctive (k_hamming.hip).  Observation j of a point
//                   resolves through the call's key-frame table (descriptor base, keypoint base, camera centre, flags) to the
//                   resident feature set: nothing is staged.  Descriptor half: lane i owns row i of the distance matrix of the
//                   observers that are not bad (rows beyond 16 in further rounds), the row median by bisection on the value,
//                   min over median << 20 | position.  Normal half: each lane forms its observers' scaled viewing directions, the
//                   running sum is added in list order through a shuffle chain (docs/parity.md: order-dependent loops keep their
//                   order).  Lane 0 writes geoA.w, geoB and the descriptor slot; flag word and generation are not touched.  The
//                   kernel reads descriptors only from sets and positions only from geoA.xyz, and a slot occurs once per call, so
//                   writing inside the launch is safe.
//   k_map_gather    store entries by slot into one result block (orbhip_map_get).
// Every float / double operation is individually rounded (docs/parity.md, "UpdateNormalAndDepth").
#include "refresh_dev.h"   // the normal half: normal_and_depth, shared with k_correct.hip

__global__ __launch_bounds__(256) void k_map_refresh(const RefreshKfDev *__restrict__ kfs, const orbhip_refresh_params *__restrict__ prm,
                                                     const int32_t *__restrict__ slots, const int32_t *__restrict__ off,
                                                     const int2 *__restrict__ obs, const int32_t *__restrict__ refPos, int P,
                                                     int maxPoints, float4 *geoA, float4 *geoB, const uint32_t *__restrict__ mflags,
                                                     uint4 *mdesc, uint8_t *__restrict__ status, int32_t *__restrict__ bestPos,
                                                     uint4 *__restrict__ descOut, float4 *__restrict__ geoBOut,
                                                     float *__restrict__ minOut)
{
    const int p = blockIdx.x * 16 + (threadIdx.x >> 4), lane = threadIdx.x & 15;
    if (p >= P) return;
    const int slot = slots[p];
    if (slot < 0 || slot >= maxPoints) return;   // (the host resolves every key before the launch)
    const int s = off[p], N = off[p + 1] - s;
    const uint32_t fl = mflags[slot];
    const float4 A = geoA[slot];
    float4 B = geoB[slot];
    float minDist = A.w;
    uint4 D0 = mdesc[2 * (size_t)slot], D1 = mdesc[2 * (size_t)slot + 1];
    const int what = prm->what;
    const bool live = !(fl & ORBHIP_MP_BAD) && N > 0;
    int st = 0, best = -1;

    if (live && (what & ORBHIP_REFRESH_DESC)) {
        int nb = 0;   // observers that are not bad
        for (int j = lane; j < N; j += 16) nb += (kfs[obs[s + j].x].flags & ORBHIP_KF_BAD) ? 0 : 1;
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) nb += __shfl_xor(nb, d);
        if (nb > 0) {
            const int k = (int)(0.5 * (double)(nb - 1));
            unsigned key = 0xffffffffu;
            for (int i0 = 0; i0 < N; i0 += 16) {
                const int i = i0 + lane;
                if (i >= N) continue;
                const int2 oi = obs[s + i];
                if (kfs[oi.x].flags & ORBHIP_KF_BAD) continue;
                const uint4 *Di = kfs[oi.x].desc + 2 * (size_t)oi.y;
                const uint4 a0 = Di[0], a1 = Di[1];
                int lo = 0, hi = 256;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    for (int j = 0; j < N; j++) {
                        const int2 oj = obs[s + j];
                        if (kfs[oj.x].flags & ORBHIP_KF_BAD) continue;
                        const uint4 *Dj = kfs[oj.x].desc + 2 * (size_t)oj.y;
                        cnt += hamming256(a0, a1, Dj[0], Dj[1]) <= mid;
                    }
                    if (cnt > k) hi = mid;
                    else lo = mid + 1;
                }
                key = min(key, ((unsigned)lo << 20) | (unsigned)i);
            }
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, d));
            best = (int)(key & 0xfffffu);
            const int2 ob = obs[s + best];
            const uint4 *Db = kfs[ob.x].desc + 2 * (size_t)ob.y;
            D0 = Db[0], D1 = Db[1];
            st |= ORBHIP_REFRESH_DESC;
        }
    }

    if (live && (what & ORBHIP_REFRESH_NORMAL)) {
        const int2 orf = obs[s + min(max(refPos[p], 0), N - 1)];
        const int level = kfs[orf.x].kps[orf.y].octave;
        normal_and_depth(A.x, A.y, A.z, N, lane, refPos[p], level, prm,
                         [&](int j, float &ox, float &oy, float &oz) {   // the observer's centre: the one of the call's table
                             const RefreshKfDev &K = kfs[obs[s + j].x];
                             ox = K.ox, oy = K.oy, oz = K.oz;
                         },
                         B, minDist);
        st |= ORBHIP_REFRESH_NORMAL;
    }

    if (lane == 0) {
        if (st & ORBHIP_REFRESH_DESC) mdesc[2 * (size_t)slot] = D0, mdesc[2 * (size_t)slot + 1] = D1;
        if (st & ORBHIP_REFRESH_NORMAL) {
            reinterpret_cast<float *>(geoA)[4 * (size_t)slot + 3] = minDist;
            geoB[slot] = B;
        }
        status[p] = (uint8_t)st;
        bestPos[p] = best;
        descOut[2 * (size_t)p] = D0, descOut[2 * (size_t)p + 1] = D1;
        geoBOut[p] = B;
        minOut[p] = minDist;
    }
}

void launch_map_refresh(hipStream_t s, const RefreshKfDev *kfs, const orbhip_refresh_params *prm, const int32_t *slots,
                        const int32_t *off, const void *obs, const int32_t *refPos, int P, int maxPoints, void *geoA, void *geoB,
                        const uint32_t *mflags, void *mdesc, uint8_t *status, int32_t *bestPos, void *descOut, void *geoBOut,
                        float *minOut)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_map_refresh, dim3((P + 15) / 16, 1, 1), dim3(256, 1, 1), 0, s, kfs, prm, slots, off, (const int2 *)obs, refPos, P,
                       maxPoints, (float4 *)geoA, (float4 *)geoB, mflags, (uint4 *)mdesc, status, bestPos, (uint4 *)descOut,
                       (float4 *)geoBOut, minOut);
}

__global__ __launch_bounds__(256) void k_map_gather(const int32_t *__restrict__ slots, int n, int maxPoints,
                                                    const float4 *__restrict__ geoA, const float4 *__restrict__ geoB,
                                                    const uint32_t *__restrict__ mflags, const uint4 *__restrict__ mdesc,
                                                    float4 *__restrict__ aOut, float4 *__restrict__ bOut, uint4 *__restrict__ descOut,
                                                    uint32_t *__restrict__ flagsOut)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s < 0 || s >= maxPoints) return;
    aOut[i] = geoA[s];
    bOut[i] = geoB[s];
    descOut[2 * (size_t)i] = mdesc[2 * (size_t)s];
    descOut[2 * (size_t)i + 1] = mdesc[2 * (size_t)s + 1];
    flagsOut[i] = mflags[s];
}

void launch_map_gather(hipStream_t s, const int32_t *slots, int n, int maxPoints, const void *geoA, const void *geoB,
                       const uint32_t *mflags, const void *mdesc, void *aOut, void *bOut, void *descOut, uint32_t *flagsOut)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_map_gather, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slots, n, maxPoints, (const float4 *)geoA,
                       (const float4 *)geoB, mflags, (const uint4 *)mdesc, (float4 *)aOut, (float4 *)bOut, (uint4 *)descOut, flagsOut);
}
