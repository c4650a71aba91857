// k_loopfuse.hip -- what LoopClosing's two projection searches need beside the kernels of k_fuse.hip (ref: src/ORBmatcher.cc:290-403,
// :977-1100, src/LoopClosing.cc:404-427, :647-673): "the target key frame holds this point already"
// (spAlreadyFound = pKF->GetMapPoints(), :993, :1005) for K targets, taken from the key-frame table on the device.
//   k_mark_index   the loop list leaves "position in the list + 1" in the mark word of each of its slots
//   k_loop_held    one lane per (target, entry of the target's row): the entry resolves through kf_entry_slot (live, not bad, the
//                  entry's generation -- a stale entry whose slot went to another point of the list resolves to nothing), the
//                  slot's mark word names the list position, and skip[target][position] is set
// The marks are cleared again by k_mark_clear (k_localcollect.hip) over the same list.  k_project_fuse<false, true> then reads the
// skip bytes.  The list holds no slot twice (the caller refuses a key twice), so every mark word has one writer.
#include "localmap_dev.h"

__global__ __launch_bounds__(256) void k_mark_index(const int32_t *__restrict__ slots, int n, int maxPoints, uint32_t *__restrict__ marks)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s >= 0 && s < maxPoints) marks[s] = (uint32_t)i + 1u;
}

// rowIdx [K]: the target's row in the table, or -1 (no such test); skip [K][n], zero on entry
__global__ __launch_bounds__(256) void k_loop_held(const int2 *__restrict__ rows, int stride, int maxRow, const int32_t *__restrict__ rowIdx,
                                                   const uint32_t *__restrict__ mflags, int maxPoints,
                                                   const uint32_t *__restrict__ marks, int n, uint8_t *__restrict__ skip)
{
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    const int r = rowIdx[b];
    if (r < 0) return;   // block-uniform
    const int2 *row = rows + (size_t)r * stride;
    if (e >= min(row[0].x, maxRow)) return;
    const int s = kf_entry_slot(row[1 + e], mflags, maxPoints);
    if (s < 0) return;
    const uint32_t m = marks[s];
    if (m >= 1u && m <= (uint32_t)n) skip[(size_t)b * n + (m - 1u)] = 1;
}

// slots [n] (device): the loop list; maxLen = the longest of the K rows; marks are zero on entry and zero again when the chain has run
void launch_loop_held(hipStream_t s, const void *rows, int stride, int maxRow, const int32_t *rowIdx, int K, int maxLen,
                      const uint32_t *mflags, int maxPoints, uint32_t *marks, const int32_t *slots, int n, uint8_t *skip)
{
    if (n <= 0 || K <= 0 || maxLen <= 0) return;
    hipLaunchKernelGGL(k_mark_index, dim3((n + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, slots, n, maxPoints, marks);
    hipLaunchKernelGGL(k_loop_held, dim3((maxLen + 255) / 256, K, 1), dim3(256, 1, 1), 0, s, (const int2 *)rows, stride, maxRow, rowIdx,
                       mflags, maxPoints, marks, n, skip);
    launch_mark_clear(s, slots, n, maxPoints, marks);
}
