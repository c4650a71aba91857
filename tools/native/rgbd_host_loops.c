/* What orbhip_frame_build_rgbd takes off a host core (tools/rgbd_latency.py compiles this with -O3 -march=native and times it):
 * the grey conversion of a packed RGB frame and the conversion of a whole 16-bit depth map to float, as plain loops. */
#include <stdint.h>

void host_grey_rgb(const uint8_t *src, int w, int h, int stride, uint8_t *dst, int dstride)
{
    for (int y = 0; y < h; y++) {
        const uint8_t *s = src + (long)y * stride;
        uint8_t *d = dst + (long)y * dstride;
        for (int x = 0; x < w; x++) d[x] = (uint8_t)((4899 * s[3 * x] + 9617 * s[3 * x + 1] + 1868 * s[3 * x + 2] + 8192) >> 14);
    }
}

void host_convert_u16(const uint16_t *src, int n, float factor, float *dst)
{
    for (int i = 0; i < n; i++) dst[i] = (float)src[i] * factor;
}
