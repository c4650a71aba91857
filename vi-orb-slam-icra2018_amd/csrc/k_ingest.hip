// k_ingest.hip -- what stands in front of the extractor for a colour / RGB-D camera
// (ref: src/Tracking.cc:904-932 GrabImageRGBD; the same cvtColor heads GrabImageStereo and GrabImageMonocular):
//   k_grey         cvtColor(im, im, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) on packed 8-bit pixels, B frames;
//   k_rgbd_depth   Frame::ComputeStereoFromRGBD (ref: src/Frame.cc:987-1008) with the imDepth.convertTo in front of it
//                  (ref: src/Tracking.cc:924-925) evaluated at the one pixel each keypoint reads, one lane per keypoint.
// The arithmetic: OpenCV 2.4's RGB2Gray<uchar>, grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 in
// integers (its three tables hold exactly these products, the bias in the first one); at most 255 * 16384 + 8192, so nothing
// saturates.  The depth: rgbd_depth.h.
#include "orbhip_internal.h"
#include "rgbd_depth.h"

#define GREY_CG 9617u
#define GREY_BIAS 8192u
#define GREY_SHIFT 14

// (dword loads of 4-byte alignment: a row of packed RGB starts on a dword, not on 12 or 16 bytes)
struct alignas(4) GreyIn3 { uint32_t a, b, c; };
struct alignas(4) GreyIn4 { uint32_t a, b, c, d; };

__device__ __forceinline__ uint32_t grey_of(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t c0, uint32_t c2)
{
    return (c0 * p0 + GREY_CG * p1 + c2 * p2 + GREY_BIAS) >> GREY_SHIFT;
}
__device__ __forceinline__ uint32_t byte_of(uint32_t v, int k) { return (v >> (8 * k)) & 255u; }

// One lane = four neighbouring pixels of one row: three (RGB) or four (RGBA) dwords in, one dword out.  c0 / c2 weigh the first
// and the third byte of a pixel (4899 and 1868, swapped for BGR); the fourth byte is never looked at.  A streaming kernel:
// (CH + 1) bytes of traffic per pixel and a dozen integer operations.  Byte by byte instead: the last w % 4 pixels of a row, and
// every row that does not start on a dword on both sides (packed RGB of a width that is not a multiple of 4, from the host forms;
// the device form asks for aligned rows).
template <int CH>
__global__ __launch_bounds__(256) void k_grey(const uint8_t *__restrict__ src, int w, int h, int stride, size_t sframe, uint32_t c0,
                                              uint32_t c2, uint8_t *__restrict__ dst, int dstride, size_t dframe)
{
    const unsigned G = ((unsigned)w + 3u) >> 2;   // lanes per row
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const unsigned y = idx / G;
    if (y >= (unsigned)h) return;
    const unsigned x = (idx - y * G) * 4u;
    const uint8_t *S = src + (size_t)blockIdx.y * sframe + (size_t)y * stride;
    uint8_t *D = dst + (size_t)blockIdx.y * dframe + (size_t)y * dstride;
    if (x + 4u <= (unsigned)w && ((((uintptr_t)S) | ((uintptr_t)D)) & 3u) == 0) {
        uint32_t g0, g1, g2, g3;
        if (CH == 3) {
            const GreyIn3 v = *reinterpret_cast<const GreyIn3 *>(S + (size_t)x * 3);
            g0 = grey_of(byte_of(v.a, 0), byte_of(v.a, 1), byte_of(v.a, 2), c0, c2);
            g1 = grey_of(byte_of(v.a, 3), byte_of(v.b, 0), byte_of(v.b, 1), c0, c2);
            g2 = grey_of(byte_of(v.b, 2), byte_of(v.b, 3), byte_of(v.c, 0), c0, c2);
            g3 = grey_of(byte_of(v.c, 1), byte_of(v.c, 2), byte_of(v.c, 3), c0, c2);
        } else {
            const GreyIn4 v = *reinterpret_cast<const GreyIn4 *>(S + (size_t)x * 4);
            g0 = grey_of(byte_of(v.a, 0), byte_of(v.a, 1), byte_of(v.a, 2), c0, c2);
            g1 = grey_of(byte_of(v.b, 0), byte_of(v.b, 1), byte_of(v.b, 2), c0, c2);
            g2 = grey_of(byte_of(v.c, 0), byte_of(v.c, 1), byte_of(v.c, 2), c0, c2);
            g3 = grey_of(byte_of(v.d, 0), byte_of(v.d, 1), byte_of(v.d, 2), c0, c2);
        }
        *reinterpret_cast<uint32_t *>(D + x) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        return;
    }
    const unsigned xe = min(x + 4u, (unsigned)w);
    for (unsigned i = x; i < xe; i++) {
        const uint8_t *p = S + (size_t)i * CH;
        D[i] = (uint8_t)grey_of(p[0], p[1], p[2], c0, c2);
    }
}

void launch_grey(hipStream_t s, const uint8_t *src, int B, int w, int h, int stride, size_t sframe, int channels, bool bgr,
                 uint8_t *dst, int dstride, size_t dframe)
{
    const unsigned lanes = (((unsigned)w + 3u) >> 2) * (unsigned)h;
    const dim3 grid((lanes + 255u) / 256u, (unsigned)B);
    const uint32_t c0 = bgr ? 1868u : 4899u, c2 = bgr ? 4899u : 1868u;
    if (channels == 3)
        hipLaunchKernelGGL(k_grey<3>, grid, dim3(256), 0, s, src, w, h, stride, sframe, c0, c2, dst, dstride, dframe);
    else
        hipLaunchKernelGGL(k_grey<4>, grid, dim3(256), 0, s, src, w, h, stride, sframe, c0, c2, dst, dstride, dframe);
}

// Rows [counts[b], cap) of the outputs are left alone.
__global__ __launch_bounds__(256) void k_rgbd_depth(const orbhip_keypoint *__restrict__ kps, const orbhip_keypoint *__restrict__ kpsUn,
                                                    const int32_t *__restrict__ counts, int cap, const uint8_t *__restrict__ depth,
                                                    int depthType, int dw, int dh, size_t dstride, size_t dframe, float factor,
                                                    int scales, float mbf, float *__restrict__ uRight, float *__restrict__ depthOut)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = counts ? min(counts[b], cap) : cap;
    if (i >= n) return;
    const size_t k = (size_t)b * cap + i;
    orb_rgbd_depth_one(kps[k].x, kps[k].y, kpsUn[k].x, depth + (size_t)b * dframe, depthType, dw, dh, dstride, factor, scales != 0,
                       mbf, &uRight[k], &depthOut[k]);
}

void launch_rgbd_depth(hipStream_t s, const orbhip_keypoint *kps, const orbhip_keypoint *kpsUn, const int32_t *counts, int cap, int B,
                       const void *depth, int depthType, int dw, int dh, size_t dstride, size_t dframe, float factor, float mbf,
                       float *uRight, float *depthOut)
{
    hipLaunchKernelGGL(k_rgbd_depth, dim3((cap + 255) / 256, B), dim3(256), 0, s, kps, kpsUn, counts, cap, (const uint8_t *)depth,
                       depthType, dw, dh, dstride, dframe, factor, orb_rgbd_scales(depthType, factor) ? 1 : 0, mbf, uRight, depthOut);
}
