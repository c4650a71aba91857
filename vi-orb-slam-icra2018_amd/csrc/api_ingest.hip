// api_ingest.hip -- C ABI, part 11: colour frames in, depth at the keypoints out (the RGB-D sensor path).
//
// Tracking::GrabImageRGBD (ref: src/Tracking.cc:904-932) converts the colour frame to grey and the whole depth map to float on a
// host core, then builds the Frame, whose constructor reads the float map at the keypoints (ref: src/Frame.cc:987-1008).  Here
//   * the colour frame is what travels: k_grey (k_ingest.hip) is the first node of the single-frame graphs, in front of the
//     unchanged chain of orbhip_extract / orbhip_frame_build;
//   * the single-frame calls gather the depth on the host, after their one synchronisation: n reads of the caller's map and
//     three float operations each (rgbd_depth.h), where an upload would move 614 KB to read a thousand samples;
//   * batches whose frames, keypoints and depth maps are resident have orbhip_grey_device and orbhip_rgbd_depth_device.
#include "api_common.h"
#include "rgbd_depth.h"

int orb_format_channels(int format)
{
    switch (format) {
    case ORBHIP_FMT_GREY: return 1;
    case ORBHIP_FMT_RGB: case ORBHIP_FMT_BGR: return 3;
    case ORBHIP_FMT_RGBA: case ORBHIP_FMT_BGRA: return 4;
    }
    return 0;
}
static bool format_bgr(int format) { return format == ORBHIP_FMT_BGR || format == ORBHIP_FMT_BGRA; }
static bool is_colour(int format) { return format != ORBHIP_FMT_GREY && orb_format_channels(format) != 0; }
static int depth_elem(int depth_type) { return depth_type == ORBHIP_DEPTH_U16 ? 2 : depth_type == ORBHIP_DEPTH_F32 ? 4 : 0; }

// The caller's colour frame -> the page-locked block, rows packed (w * channels bytes apart: what crosses the bus is the pixels).
// The graphs that hold the two blocks have their addresses in their replay keys.
int orb_color_stage(orbhip_ctx *c, const uint8_t *img, int w, int h, int stride, int format)
{
    const size_t row = (size_t)w * orb_format_channels(format), bytes = row * h;
    if (bytes > c->h_color.bytes()) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the last call's copy has long finished; its graph goes with the key)
        HIPCHK(c, c->h_color.grow(bytes));
        HIPCHK(c, c->d_color.grow(bytes));
    }
    int rc;
    if (c->hostPyr && (rc = orb_host_in_stage(c, c->lvl0FrameBytes))) return rc;
    uint8_t *dst = c->h_color.as<uint8_t>();
    if ((size_t)stride == row)
        memcpy(dst, img, bytes);
    else
        for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * row, img + (size_t)y * stride, row);
    return ORBHIP_OK;
}

// copy in, k_grey into the context's level-0 buffer at stride s0; with the host pyramid on, level 0 -- the grey image, which the
// caller never had -- goes back to c->h_in, where orbhip_host_pyramid_level looks for it
int orb_color_enqueue(orbhip_ctx *c, int w, int h, int format, int s0)
{
    const int ch = orb_format_channels(format);
    const size_t bytes = (size_t)w * ch * h;
    HIPCHK(c, hipMemcpyAsync(c->d_color.as<uint8_t>(), c->h_color.as<uint8_t>(), bytes, hipMemcpyHostToDevice, c->stream));
    launch_grey(c->stream, c->d_color.as<uint8_t>(), 1, w, h, w * ch, bytes, ch, format_bgr(format), c->d_lvl0.as<uint8_t>(), s0,
                c->lvl0FrameBytes);
    HIPCHK(c, hipGetLastError());
    if (c->hostPyr)
        HIPCHK(c, hipMemcpyAsync(c->h_in.as<uint8_t>(), c->d_lvl0.as<uint8_t>(), (size_t)s0 * (h - 1) + w, hipMemcpyDeviceToHost,
                                 c->stream));
    return ORBHIP_OK;
}

static bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

extern "C" int orbhip_grey_device(orbhip_ctx *c, const void *d_src, int B, int w, int h, int stride, size_t frame_stride, int format,
                                  void *d_dst, int dst_stride, size_t dst_frame_stride)
{
    if (!c || !d_src || !d_dst || B <= 0 || B > 65535 || w <= 0 || h <= 0)
        return fail(c, ORBHIP_E_ARG, "orbhip_grey_device: bad argument");
    if (!is_colour(format)) return fail(c, ORBHIP_E_ARG, "orbhip_grey_device: format must be one of ORBHIP_FMT_RGB, _BGR, _RGBA, _BGRA");
    const int ch = orb_format_channels(format);
    if ((long long)stride < (long long)w * ch || dst_stride < w)
        return fail(c, ORBHIP_E_ARG, "orbhip_grey_device: stride smaller than a row (w * channels source bytes, w destination bytes)");
    if (!aligned4(d_src) || !aligned4(d_dst) || stride % 4 || dst_stride % 4 || frame_stride % 4 || dst_frame_stride % 4)
        return fail(c, ORBHIP_E_ARG, "orbhip_grey_device: bases must be 4-byte aligned and every stride a multiple of 4");
    if (B > 1 && dst_frame_stride < (size_t)dst_stride * (h - 1) + w)
        return fail(c, ORBHIP_E_ARG, "orbhip_grey_device: destination frames overlap");
    HIPCHK(c, orb_enter(c));
    launch_grey(c->stream, (const uint8_t *)d_src, B, w, h, stride, frame_stride, ch, format_bgr(format), (uint8_t *)d_dst, dst_stride,
                dst_frame_stride);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_grey(orbhip_ctx *c, const uint8_t *src, int w, int h, int stride, int format, uint8_t *dst, int dst_stride)
{
    if (!c || !src || !dst || w <= 0 || h <= 0) return fail(c, ORBHIP_E_ARG, "orbhip_grey: bad argument");
    if (!is_colour(format)) return fail(c, ORBHIP_E_ARG, "orbhip_grey: format must be one of ORBHIP_FMT_RGB, _BGR, _RGBA, _BGRA");
    const int ch = orb_format_channels(format);
    if ((long long)stride < (long long)w * ch || dst_stride < w)
        return fail(c, ORBHIP_E_ARG, "orbhip_grey: stride smaller than a row (w * channels source bytes, w destination bytes)");
    HIPCHK(c, orb_enter(c));
    // packed rows on the device: the pixels are all that crosses the bus; grey rows on a dword each
    const size_t row = (size_t)w * ch, gstride = align_up((size_t)w, 4);
    TmpDev T(c);
    int rc;
    if ((rc = T.reserve(row * h + gstride * h + 512))) return rc;
    uint8_t *dIn = (uint8_t *)T.take(row * h), *dOut = (uint8_t *)T.take(gstride * h);
    TMPCHK(c, T);
    HIPCHK(c, hipMemcpy2DAsync(dIn, row, src, (size_t)stride, row, (size_t)h, hipMemcpyHostToDevice, c->stream));
    launch_grey(c->stream, dIn, 1, w, h, (int)row, row * h, ch, format_bgr(format), dOut, (int)gstride, gstride * h);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dst_stride, dOut, gstride, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ORBHIP_OK;
}

extern "C" int orbhip_extract_color(orbhip_ctx *c, const uint8_t *img, int w, int h, int stride, int format, orbhip_keypoint *kps,
                                    uint8_t *desc, int cap, int *n_out, float timings_ms[3])
{
    if (format == ORBHIP_FMT_GREY) return orbhip_extract(c, img, w, h, stride, kps, desc, cap, n_out, timings_ms);
    if (!c || !img || !kps || !desc || !n_out || cap <= 0 || w <= 0 || h <= 0)
        return fail(c, ORBHIP_E_ARG, "orbhip_extract_color: bad argument");
    if (!is_colour(format)) return fail(c, ORBHIP_E_ARG, "orbhip_extract_color: unknown format");
    if ((long long)stride < (long long)w * orb_format_channels(format))
        return fail(c, ORBHIP_E_ARG, "orbhip_extract_color: stride smaller than w * channels");
    const uint8_t *imgs[1] = {img};
    int rc = orb_extract_host(c, imgs, 1, w, h, stride, format, kps, desc, cap, n_out);
    if (rc == ORBHIP_OK && timings_ms) {
        float ms[6];
        if ((rc = orbhip_get_stage_times(c, ms))) return rc;
        timings_ms[0] = ms[0];
        timings_ms[1] = ms[1] + ms[2];
        timings_ms[2] = ms[3] + ms[4];
    }
    return rc;
}

// what the host and the device form ask of a depth map
static int depth_args_ok(orbhip_ctx *c, const char *who, const void *depth, int depth_type, int dw, int dh, long long depth_stride,
                         float factor)
{
    const int el = depth_elem(depth_type);
    if (!el) return fail(c, ORBHIP_E_ARG, std::string(who) + ": depth type must be ORBHIP_DEPTH_U16 or ORBHIP_DEPTH_F32");
    if (!depth || dw <= 0 || dh <= 0) return fail(c, ORBHIP_E_ARG, std::string(who) + ": no depth map");
    if (depth_stride < (long long)dw * el) return fail(c, ORBHIP_E_ARG, std::string(who) + ": depth stride smaller than a row");
    if (!std::isfinite(factor)) return fail(c, ORBHIP_E_ARG, std::string(who) + ": depth factor is not finite");
    return ORBHIP_OK;
}

extern "C" int orbhip_rgbd_depth(orbhip_ctx *c, const orbhip_keypoint *kps, const orbhip_keypoint *kps_un, int n, const void *depth,
                                 int depth_type, int dw, int dh, int depth_stride, float factor, float mbf, float *u_right,
                                 float *depth_out)
{
    if (n < 0 || (n > 0 && (!kps || !kps_un || !u_right || !depth_out))) return fail(c, ORBHIP_E_ARG, "orbhip_rgbd_depth: bad argument");
    if (const int rc = depth_args_ok(c, "orbhip_rgbd_depth", depth, depth_type, dw, dh, depth_stride, factor)) return rc;
    const bool scales = orb_rgbd_scales(depth_type, factor);
    for (int i = 0; i < n; i++)
        orb_rgbd_depth_one(kps[i].x, kps[i].y, kps_un[i].x, depth, depth_type, dw, dh, (size_t)depth_stride, factor, scales, mbf,
                           &u_right[i], &depth_out[i]);
    return ORBHIP_OK;
}

extern "C" int orbhip_rgbd_depth_device(orbhip_ctx *c, const void *d_kps, const void *d_kps_un, const void *d_counts, int cap, int B,
                                        const void *d_depth, int depth_type, int dw, int dh, int depth_stride,
                                        size_t depth_frame_stride, float factor, float mbf, void *d_u_right, void *d_depth_out)
{
    if (!c || !d_kps || !d_kps_un || !d_u_right || !d_depth_out || cap <= 0 || B <= 0 || B > 65535)
        return fail(c, ORBHIP_E_ARG, "orbhip_rgbd_depth_device: bad argument");
    if (const int rc = depth_args_ok(c, "orbhip_rgbd_depth_device", d_depth, depth_type, dw, dh, depth_stride, factor)) return rc;
    const int el = depth_elem(depth_type);
    if ((uintptr_t)d_depth % el || depth_stride % el || depth_frame_stride % el || !aligned4(d_kps) || !aligned4(d_kps_un) ||
        !aligned4(d_counts) || !aligned4(d_u_right) || !aligned4(d_depth_out))
        return fail(c, ORBHIP_E_ARG, "orbhip_rgbd_depth_device: a pointer or stride is not aligned to its element");
    HIPCHK(c, orb_enter(c));
    launch_rgbd_depth(c->stream, (const orbhip_keypoint *)d_kps, (const orbhip_keypoint *)d_kps_un, (const int32_t *)d_counts, cap, B,
                      d_depth, depth_type, dw, dh, (size_t)depth_stride, depth_frame_stride, factor, mbf, (float *)d_u_right,
                      (float *)d_depth_out);
    HIPCHK(c, hipGetLastError());
    return ORBHIP_OK;
}

extern "C" int orbhip_frame_build_rgbd(orbhip_ctx *c, const orbhip_frame_input *in, const orbhip_frame_params *fp, orbhip_keypoint *kps,
                                       orbhip_keypoint *kps_un, uint8_t *desc, int cap, int *n_out, int32_t *cell_off,
                                       int32_t *cell_idx, int32_t *word_id, float *weight, int32_t *node_id, float *u_right,
                                       float *depth_out)
{
    if (!c || !in || !in->img || in->w <= 0 || in->h <= 0 || (in->depth_type != ORBHIP_DEPTH_NONE && (!u_right || !depth_out)))
        return fail(c, ORBHIP_E_ARG, "orbhip_frame_build_rgbd: bad argument");
    if (!orb_format_channels(in->format)) return fail(c, ORBHIP_E_ARG, "orbhip_frame_build_rgbd: unknown format");
    if ((long long)in->stride < (long long)in->w * orb_format_channels(in->format))
        return fail(c, ORBHIP_E_ARG, "orbhip_frame_build_rgbd: stride smaller than w * channels");
    if (in->depth_type != ORBHIP_DEPTH_NONE)
        if (const int rc = depth_args_ok(c, "orbhip_frame_build_rgbd", in->depth, in->depth_type, in->w, in->h, in->depth_stride,
                                         in->depth_factor))
            return rc;
    int rc = orb_frame_build(c, in->img, in->w, in->h, in->stride, in->format, fp, kps, kps_un, desc, cap, n_out, cell_off, cell_idx,
                             word_id, weight, node_id);
    if (rc) return rc;
    const int n = *n_out;
    if (in->depth_type == ORBHIP_DEPTH_NONE) {
        for (int i = 0; i < n && u_right; i++) u_right[i] = -1.0f;
        for (int i = 0; i < n && depth_out; i++) depth_out[i] = -1.0f;
        return ORBHIP_OK;
    }
    return orbhip_rgbd_depth(c, kps, kps_un, n, in->depth, in->depth_type, in->w, in->h, in->depth_stride, in->depth_factor, in->mbf,
                             u_right, depth_out);
}
