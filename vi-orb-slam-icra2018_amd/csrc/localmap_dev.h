// localmap_dev.h -- device helpers shared by the kernels that read the resident map-point store (k_localcollect.hip, k_covis.hip,
// k_cull.hip, k_baproblem.hip, k_loopfuse.hip; k_localmap.hip, k_projtrack.hip, k_fuse.hip and k_sim3search.hip through
// project_dev.h, k_refresh.hip and k_correct.hip through refresh_dev.h, k_bowcand.hip and k_hamming.hip through bow_match_dev.h) and by the
// window searches (k_guided.hip, k_fuse.hip): the flag-word rules, the reference's gemm, the key-frame row entry, the per-batch
// count of active queries, the cell window of GetFeaturesInArea, the chi-square gate that k_window_best and window_row_best share
// and the 16-lane window walk that k_window_best_row and k_window_best_sets share.  The steps of a projection are project_dev.h's.
#ifndef ORBHIP_LOCALMAP_DEV_H
#define ORBHIP_LOCALMAP_DEV_H
#include "orbhip_internal.h"
#include "wave_ops.h"

// flag word of a slot: bits 0..1 ORBHIP_MP_*, bit 7 live, bits 8..31 the slot's generation (api_localmap.hip)
#define MP_LIVE 0x80u

// (R row) * P + t of the gemm: products and sums in double, in column order from 0.0, one rounding to float
__device__ __forceinline__ float gemm_row(const float *__restrict__ R, float t, float x, float y, float z)
{
    double s = __dadd_rn(0.0, __dmul_rn((double)R[0], (double)x));
    s = __dadd_rn(s, __dmul_rn((double)R[1], (double)y));
    s = __dadd_rn(s, __dmul_rn((double)R[2], (double)z));
    return (float)__dadd_rn(s, (double)t);
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the slot an entry names, or -1: empty, out of range, erased, re-used (another generation) or bad
__device__ __forceinline__ int kf_entry_slot(const int2 e, const uint32_t *__restrict__ mflags, int maxPoints)
{
    if (e.x < 0 || e.x >= maxPoints) return -1;
    const uint32_t fl = mflags[e.x];
    if (!(fl & MP_LIVE) || (fl & ORBHIP_MP_BAD) || (fl >> 8) != (uint32_t)e.y) return -1;
    return e.x;
}

// active queries of frame / target b: a ballot and one atomic per wave (every lane of the block arrives here)
__device__ __forceinline__ void count_active(bool active, int32_t *__restrict__ counter)
{
    const unsigned long long m = __ballot(active);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, __popcll(m));
}

#define WAVE_LDS_SYNC()                                        \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

struct GridParams {
    float minX, minY, invW, invH;
};

// The window of GetFeaturesInArea in cells; false = the early returns of src/Frame.cc:676-691.
__device__ __forceinline__ bool window_cells(const GridParams &gp, float x, float y, float r, int &x0, int &x1, int &y0,
                                             int &y1)
{
    x0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, gp.minX), r), gp.invW)));
    if (x0 >= ORBHIP_GRID_COLS) return false;
    x1 = min(ORBHIP_GRID_COLS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, gp.minX), r), gp.invW)));
    if (x1 < 0) return false;
    y0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, gp.minY), r), gp.invH)));
    if (y0 >= ORBHIP_GRID_ROWS) return false;
    y1 = min(ORBHIP_GRID_ROWS - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, gp.minY), r), gp.invH)));
    if (y1 < 0) return false;
    return true;
}

// The chi-square gate of Fuse's window loop on the reprojection error of the feature at (x, y) (ref: src/ORBmatcher.cc:915-934):
// e2 * invSigma2 <= 5.99, or <= 7.8 with the right coordinate when the feature has one (ur >= 0; pass a negative value for none).
// Individually rounded float operations; the float product is compared as a double.
__device__ __forceinline__ bool chi2_gate(const orbhip_proj_query &q, float x, float y, float ur, float invSigma2)
{
    const float ex = __fsub_rn(q.u, x), ey = __fsub_rn(q.v, y);
    float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    double lim = 5.99;
    if (ur >= 0) {
        const float er = __fsub_rn(q.proj_xr, ur);
        e2 = __fadd_rn(e2, __fmul_rn(er, er));
        lim = 7.8;
    }
    return !((double)__fmul_rn(e2, invSigma2) > lim);
}

// One 16-lane row walks the window [x0, x1] x [y0, y1] of one point (ref: src/ORBmatcher.cc:887-950): the cells' runs of the
// grid-ordered records R are laid end to end through a row scan, lane gl takes every 16th feature.  The geometric filter, the
// level window, the chi-square gate (chi2_gate, with UR[idx] when there is a UR) and the Hamming distance to (a0, a1).
// key = the lane's smallest (distance << 20 | position in visiting order), idx = that feature.  sStart[16], sExcl[17]: the row's LDS.  Row-uniform control flow.
template <typename SIGMA>
__device__ __forceinline__ void window_row_best(const orbhip_proj_query &q, int x0, int x1, int y0, int y1, const uint4 a0,
                                                const uint4 a1, const uint4 *__restrict__ D, const float *__restrict__ UR,
                                                const float4 *__restrict__ R, const int32_t *__restrict__ O, bool gateOn,
                                                SIGMA invSigma2, int *sStart, int *sExcl, int gl, int &key, int &myIdx)
{
    int seen = 0;
    for (int cb = x0; cb <= x1; cb += 16) {
        const int ix = cb + gl;
        const int s = ix <= x1 ? O[ix * ORBHIP_GRID_ROWS + y0] : 0, e = ix <= x1 ? O[ix * ORBHIP_GRID_ROWS + y1 + 1] : 0;
        const int incl = row_incl_scan(e - s);
        sStart[gl] = s;
        sExcl[gl + 1] = incl;
        if (gl == 0) sExcl[0] = 0;
        WAVE_LDS_SYNC();
        const int total = sExcl[16];
        for (int r = gl; r < total; r += 16) {
            int c = 0;
#pragma unroll
            for (int h = 8; h > 0; h >>= 1)
                if (sExcl[c + h] <= r) c += h;
            const float4 rr = R[sStart[c] + (r - sExcl[c])];
            const int w = __float_as_int(rr.z), oct = w & 255, idx = w >> 8;
            if (!(fabsf(__fsub_rn(rr.x, q.u)) < q.radius && fabsf(__fsub_rn(rr.y, q.v)) < q.radius)) continue;
            if (oct < q.min_level || oct > q.max_level) continue;
            if (gateOn && !chi2_gate(q, rr.x, rr.y, UR ? UR[idx] : -1.0f, invSigma2(oct))) continue;
            const int d = hamming256(a0, a1, D[2 * idx], D[2 * idx + 1]);
            const int k = (d << 20) | (seen + r);
            if (d < 256 && k < key) {
                key = k;
                myIdx = idx;
            }
        }
        seen += total;
        WAVE_LDS_SYNC();
    }
}

// the row's minimum -> *bestIdx, *bestDist (-1 / 256 when no lane found a feature); every lane of the row arrives here
__device__ __forceinline__ void window_row_store(int key, int myIdx, int gl, int32_t *__restrict__ bestIdx,
                                                 int32_t *__restrict__ bestDist)
{
    const int k1 = row_min_inactive_ok(key);
    if (key == k1 && k1 != 0x7FFFFFFF) {   // one lane: positions are unique
        *bestIdx = myIdx;
        *bestDist = k1 >> 20;
    }
    if (k1 == 0x7FFFFFFF && gl == 0) {
        *bestIdx = -1;
        *bestDist = 256;
    }
}

#endif
