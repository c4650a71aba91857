"""Python mirror of the RGB-D sensor path (include/orbhip.h, orbhip_grey* / orbhip_extract_color / orbhip_rgbd_depth* /
orbhip_frame_build_rgbd): colour frames in, depth at the keypoints out.  All arithmetic runs in liborbhip."""
import ctypes as C

import numpy as np

from . import capi
from .capi import KP_DTYPE, _p, check

f32 = np.float32
FMT_GREY, FMT_RGB, FMT_BGR, FMT_RGBA, FMT_BGRA = range(5)
DEPTH_NONE, DEPTH_U16, DEPTH_F32 = range(3)
CHANNELS = {FMT_GREY: 1, FMT_RGB: 3, FMT_BGR: 3, FMT_RGBA: 4, FMT_BGRA: 4}


class FrameInput(C.Structure):   # orbhip_frame_input
    _fields_ = [("img", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("stride", C.c_int), ("format", C.c_int),
                ("depth", C.c_void_p), ("depth_type", C.c_int), ("depth_stride", C.c_int), ("depth_factor", C.c_float),
                ("mbf", C.c_float)]


def _image(image, fmt):
    """(array, w, h, stride) of an (H, W, channels) -- (H, W) for grey -- uint8 image whose rows may be strided."""
    a = np.asarray(image)
    ch = CHANNELS[fmt]
    assert a.dtype == np.uint8 and (a.ndim == 3 and a.shape[2] == ch or ch == 1 and a.ndim == 2)
    assert a.strides[1] == ch and (a.ndim == 2 or a.strides[2] == 1), "pixels must be packed"
    return a, a.shape[1], a.shape[0], a.strides[0]


def depth_type_of(depth):
    return {np.dtype(np.uint16): DEPTH_U16, np.dtype(np.float32): DEPTH_F32}[np.asarray(depth).dtype]


def grey(ctx, image, fmt, out=None):
    """orbhip_grey: cvtColor to grey on the device.  out: (H, W') uint8 with W' >= W, written in place (columns from W on are
    left alone); default a fresh (H, W) array."""
    a, w, h, stride = _image(image, fmt)
    if out is None:
        out = np.empty((h, w), np.uint8)
    assert out.dtype == np.uint8 and out.shape[0] == h and out.shape[1] >= w and out.strides[1] == 1
    check(capi.load().orbhip_grey(ctx.handle, C.c_void_p(a.ctypes.data), w, h, stride, fmt, C.c_void_p(out.ctypes.data),
                                  out.strides[0]), ctx.handle, "orbhip_grey")
    return out


def grey_device(ctx, d_src, B, w, h, stride, frame_stride, fmt, d_dst, dst_stride, dst_frame_stride):
    """Raw device pointers (ints / c_void_p); asynchronous."""
    check(capi.load().orbhip_grey_device(ctx.handle, d_src, B, w, h, stride, frame_stride, fmt, d_dst, dst_stride, dst_frame_stride),
          ctx.handle, "orbhip_grey_device")


def extract_color(ctx, image, fmt):
    """orbhip_extract_color: (keypoints, descriptors) of one colour frame."""
    a, w, h, stride = _image(image, fmt)
    kps, desc, n = np.zeros(ctx.cap, KP_DTYPE), np.zeros((ctx.cap, 32), np.uint8), C.c_int()
    check(capi.load().orbhip_extract_color(ctx.handle, C.c_void_p(a.ctypes.data), w, h, stride, fmt, _p(kps), _p(desc), ctx.cap,
                                           C.byref(n), None), ctx.handle, "orbhip_extract_color")
    return kps[:n.value].copy(), desc[:n.value].copy()


def rgbd_depth(kps, kps_un, depth, factor, mbf, ctx=None):
    """orbhip_rgbd_depth (host arithmetic, no device needed): (u_right, depth) of the keypoints."""
    kps, kps_un = np.ascontiguousarray(kps, KP_DTYPE), np.ascontiguousarray(kps_un, KP_DTYPE)
    d = np.asarray(depth)
    assert len(kps) == len(kps_un) and d.ndim == 2 and d.strides[1] == d.itemsize
    ur, dz = np.empty(max(len(kps), 1), f32), np.empty(max(len(kps), 1), f32)
    h = None if ctx is None else ctx.handle
    check(capi.load().orbhip_rgbd_depth(h, _p(kps), _p(kps_un), len(kps), C.c_void_p(d.ctypes.data), depth_type_of(d), d.shape[1],
                                        d.shape[0], d.strides[0], f32(factor), f32(mbf), _p(ur), _p(dz)), h, "orbhip_rgbd_depth")
    return ur[:len(kps)].copy(), dz[:len(kps)].copy()


def rgbd_depth_device(ctx, d_kps, d_kps_un, d_counts, cap, B, d_depth, depth_type, dw, dh, depth_stride, depth_frame_stride, factor,
                      mbf, d_u_right, d_depth_out):
    """Raw device pointers; asynchronous."""
    check(capi.load().orbhip_rgbd_depth_device(ctx.handle, d_kps, d_kps_un, d_counts, cap, B, d_depth, depth_type, dw, dh, depth_stride,
                                               depth_frame_stride, f32(factor), f32(mbf), d_u_right, d_depth_out), ctx.handle,
          "orbhip_rgbd_depth_device")


def frame_build_rgbd(ctx, image, fmt, depth, factor, mbf, K=None, dist_coef=None, gp=None, levelsup=-1):
    """orbhip_frame_build_rgbd: ORBextractor.frame_build's dict plus u_right and depth.  depth: (H, W) uint16 / float32, or None."""
    a, w, h, stride = _image(image, fmt)
    P = capi.FrameParams()
    Kf = np.eye(3, dtype=f32).ravel() if K is None else np.ascontiguousarray(K, f32).ravel()
    D = np.zeros(0, f32) if dist_coef is None else np.ascontiguousarray(dist_coef, f32).ravel()
    for i in range(9):
        P.K[i] = float(Kf[i])
    for i in range(len(D)):
        P.dist[i] = float(D[i])
    P.ndist = len(D)
    if gp is not None:
        P.min_x, P.min_y, P.inv_w, P.inv_h = [float(v) for v in gp]
    P.levelsup = int(levelsup)
    I = FrameInput(a.ctypes.data, w, h, stride, fmt, None, DEPTH_NONE, 0, 1.0, float(mbf))
    if depth is not None:
        d = np.asarray(depth)
        assert d.shape == (h, w) and d.strides[1] == d.itemsize
        I.depth, I.depth_type, I.depth_stride, I.depth_factor = d.ctypes.data, depth_type_of(d), d.strides[0], float(f32(factor))
    cap = ctx.cap
    kps, kun, desc = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE), np.zeros((cap, 32), np.uint8)
    off = np.zeros(capi.GRID_COLS * capi.GRID_ROWS + 1, np.int32) if gp is not None else None
    idx = np.zeros(cap, np.int32) if gp is not None else None
    word = np.zeros(cap, np.int32) if levelsup >= 0 else None
    wt = np.zeros(cap, f32) if levelsup >= 0 else None
    node = np.zeros(cap, np.int32) if levelsup >= 0 else None
    ur, dz = np.zeros(cap, f32), np.zeros(cap, f32)
    n = C.c_int()
    check(capi.load().orbhip_frame_build_rgbd(ctx.handle, C.byref(I), C.byref(P), _p(kps), _p(kun), _p(desc), cap, C.byref(n), _p(off),
                                              _p(idx), _p(word), _p(wt), _p(node), _p(ur), _p(dz)), ctx.handle,
          "orbhip_frame_build_rgbd")
    m = n.value
    cut = lambda x: None if x is None else x[:m].copy()
    if idx is not None:
        idx = idx[:off[-1]].copy()
    return dict(kps=kps[:m].copy(), kps_un=kun[:m].copy(), desc=desc[:m].copy(), cell_off=off, cell_idx=idx, word_id=cut(word),
                weight=cut(wt), node_id=cut(node), u_right=ur[:m].copy(), depth=dz[:m].copy())
