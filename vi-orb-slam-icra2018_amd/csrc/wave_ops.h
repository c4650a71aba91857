// wave_ops.h -- the one definition of each low-level wave primitive the kernels share: LDS-DMA loads, DPP prefix sums, sums
// and minima over a 16-lane row or the 64-lane wave, and the 256-bit descriptor distance.  Device code only.
// tests/test_device_helpers.py fails if the LDS-DMA asm or a row_shr DPP step is written anywhere else in csrc/.
#ifndef ORBHIP_WAVE_OPS_H
#define ORBHIP_WAVE_OPS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// LDS-DMA: each lane loads from its own global address straight into LDS at (ldsAddr + size * lane), 16 bytes per lane
// (global_load_lds_dwordx4) or 4 (global_load_lds_dword); ldsAddr must be wave-uniform.  Inline assembly because the builtin
// makes hipcc wait vmcnt(0) before every LDS access that might alias the destination, which serialises the transfers and
// drains them before the compute phase; the caller waits for the data itself.  M0 carries the LDS address.  M0 is
// compiler-reserved and not preserved around an asm statement, so it is saved, set and restored inside the one statement;
// the s_nop 0 is the hazard wait between writing M0 and the LDS-DMA that reads it.
__device__ __forceinline__ void glds16(const void *gsrc, uint32_t ldsAddr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(ldsAddr)
                 : "memory");
}
__device__ __forceinline__ void glds4(const void *gsrc, uint32_t ldsAddr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(ldsAddr)
                 : "memory");
}

// Inclusive prefix sum within each 16-lane DPP row (row_shr 1, 2, 4, 8; lanes shifted in from outside the row add 0).
__device__ __forceinline__ int row_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
    return v;
}

// Inclusive prefix sum over the 64 lanes: the row scan, then the totals of the lower rows through v_readlane.
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v = row_incl_scan(v);
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    const int row = (int)(threadIdx.x & 63) >> 4;
    return v + (row > 0 ? t0 : 0) + (row > 1 ? t1 : 0) + (row > 2 ? t2 : 0);
}

// Sum over the 64 lanes, result wave-uniform.  DPP inside each row of 16 lanes (quad swaps, half mirror, mirror), then the
// four row sums through v_readlane: no LDS round trips.
__device__ __forceinline__ int wave_sum(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

// Minimum over the 16 lanes of a DPP row (result in every lane of the row) / over the wave (a scalar).  The row steps are
// v_min_i32 with a DPP source operand: the builtin form (row_min_inactive_ok below) compiles to v_mov_b32 + s_nop +
// v_mov_b32_dpp + v_min_i32 per step, and in the one-wave kernels that use these (sequential matching semantics: their time is
// their instruction count) that was a quarter of the instructions of a feature.  Every lane of the wave must be active.
__device__ __forceinline__ int row_min(int v)
{
    asm volatile("s_nop 1\n\t"
                 "v_min_i32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_i32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_i32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\t"
                 "v_min_i32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1"
                 : "+v"(v));
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
    v = row_min(v);
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Minimum over the 16 lanes of a DPP row, result in every lane of the row: the builtin form, for code where lanes or whole
// rows of the wave may be inactive (k_window_best_row retires whole rows early and takes the minimum afterwards).  Not
// interchangeable with row_min, which needs every lane of the wave active.
__device__ __forceinline__ int row_min_inactive_ok(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    return v;
}

// Hamming distance of two 256-bit ORB descriptors (ref: src/ORBmatcher.cc:1675-1691 DescriptorDistance), as two 16-byte
// halves each or as eight words each.
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 r0, const uint4 r1)
{
    return __popc(a0.x ^ r0.x) + __popc(a0.y ^ r0.y) + __popc(a0.z ^ r0.z) + __popc(a0.w ^ r0.w) + __popc(a1.x ^ r1.x) +
           __popc(a1.y ^ r1.y) + __popc(a1.z ^ r1.z) + __popc(a1.w ^ r1.w);
}
__device__ __forceinline__ int hamming256(const uint32_t q[8], const uint32_t r[8])
{
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) d += __popc(q[k] ^ r[k]);
    return d;
}

#endif
