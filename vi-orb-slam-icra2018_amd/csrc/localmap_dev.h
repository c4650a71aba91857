// localmap_dev.h -- device helpers shared by the kernels that read the resident map-point store (k_localmap.hip,
// k_localcollect.hip, k_projtrack.hip): the flag-word rules, the reference's gemm and the key-frame row entry.
#ifndef ORBHIP_LOCALMAP_DEV_H
#define ORBHIP_LOCALMAP_DEV_H
#include "orbhip_internal.h"

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

#endif
