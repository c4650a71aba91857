"""Python mirror of the resident map-point store and of Tracking::SearchLocalPoints as one call (include/orbhip.h,
orbhip_map_* / orbhip_search_local_points).  All arithmetic runs in liborbhip."""
import ctypes as C

import numpy as np

from . import capi
from .capi import _p, check

f32 = np.float32
MP_OBSERVED, MP_BAD = 1, 2

CAMERA_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                         ("cy", "<f4"), ("mbf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"),
                         ("scale_factors", "<f4", 16), ("log_scale_factor", "<f4"), ("nlevels", "<i4"),
                         ("viewing_cos_limit", "<f4"), ("th", "<f4"), ("level_ratio", "<f4", 15),
                         ("reserved", "<i4")])   # orbhip_local_camera
POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                        ("in_view", "<i4")])     # orbhip_local_point


def camera(Rcw, tcw, Ow, fx, fy, cx, cy, mbf, bounds, scale_factors, log_scale_factor, viewing_cos_limit=0.5, th=1.0):
    """One orbhip_local_camera record; bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    c = np.zeros(1, CAMERA_DTYPE)
    c["Rcw"][0], c["tcw"][0], c["Ow"][0] = np.asarray(Rcw, f32).ravel(), np.asarray(tcw, f32).ravel(), np.asarray(Ow, f32).ravel()
    c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"] = fx, fy, cx, cy, mbf
    c["min_x"], c["max_x"], c["min_y"], c["max_y"] = bounds
    sf = np.asarray(scale_factors, f32)
    c["scale_factors"][0][:len(sf)] = sf
    c["nlevels"], c["log_scale_factor"] = len(sf), log_scale_factor
    c["viewing_cos_limit"], c["th"] = viewing_cos_limit, th
    return c


def predict_scale_table(log_scale_factor, nlevels):
    """The threshold table of PredictScale (host only): T[k] = smallest float ratio whose level exceeds k."""
    t = np.zeros(max(nlevels - 1, 1), f32)
    check(capi.load().orbhip_debug_predict_scale_table(f32(log_scale_factor), nlevels, _p(t)), None,
          "orbhip_debug_predict_scale_table")
    return t[:nlevels - 1]


class LocalMap:
    """The map points of one context (an ORBextractor, or anything with .handle): put / update_flags / erase / clear / search."""

    def __init__(self, ctx, max_points):
        self._L = capi.load()
        self._ctx = ctx
        check(self._L.orbhip_map_init(ctx.handle, max_points), ctx.handle, "orbhip_map_init")

    def info(self):
        live, cap = C.c_int(), C.c_int()
        check(self._L.orbhip_map_info(self._ctx.handle, C.byref(live), C.byref(cap)), self._ctx.handle, "orbhip_map_info")
        return live.value, cap.value

    def put(self, keys, pos, normal, min_dist, max_dist, desc, flags):
        keys = np.ascontiguousarray(keys, np.uint64)
        a = [np.ascontiguousarray(pos, f32).reshape(-1, 3), np.ascontiguousarray(normal, f32).reshape(-1, 3),
             np.ascontiguousarray(min_dist, f32), np.ascontiguousarray(max_dist, f32),
             np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), np.ascontiguousarray(flags, np.uint8)]
        assert all(len(x) == len(keys) for x in a)
        check(self._L.orbhip_map_put(self._ctx.handle, len(keys), _p(keys), *[_p(x) for x in a]), self._ctx.handle, "orbhip_map_put")

    def update_flags(self, keys, flags):
        keys, flags = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(flags, np.uint8)
        check(self._L.orbhip_map_update_flags(self._ctx.handle, len(keys), _p(keys), _p(flags)), self._ctx.handle,
              "orbhip_map_update_flags")

    def erase(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        check(self._L.orbhip_map_erase(self._ctx.handle, len(keys), _p(keys)), self._ctx.handle, "orbhip_map_erase")

    def clear(self):
        check(self._L.orbhip_map_clear(self._ctx.handle), self._ctx.handle, "orbhip_map_clear")

    def slots(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.empty(max(len(keys), 1), np.int32)
        check(self._L.orbhip_map_slots(self._ctx.handle, len(keys), _p(keys), _p(out)), self._ctx.handle, "orbhip_map_slots")
        return out[:len(keys)].copy()

    def prepare(self, cams):
        """Fills level_ratio of every camera record (for search_device)."""
        cams = np.ascontiguousarray(cams, CAMERA_DTYPE).copy()
        for i in range(len(cams)):
            check(self._L.orbhip_local_camera_prepare(self._ctx.handle, C.c_void_p(cams[i:i + 1].ctypes.data)), self._ctx.handle,
                  "orbhip_local_camera_prepare")
        return cams

    def search(self, frame_key, n, cam, keys, skip, nnratio=0.8, u_right=None, occupied=None):
        """Into the resident set frame_key of n features (0, 0: no features).  Returns (points, n_to_match, nmatches, match)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        keys, skip = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(skip, np.uint8)
        assert len(keys) == len(skip)
        ur = None if u_right is None else np.ascontiguousarray(u_right, f32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        pts = np.zeros(max(len(keys), 1), POINT_DTYPE)
        match = np.empty(max(n, 1), np.int32)
        ntm, nm = C.c_int(), C.c_int()
        check(self._L.orbhip_search_local_points(self._ctx.handle, frame_key, _p(ur), _p(occ), _p(cam), _p(keys), _p(skip), len(keys),
                                                 nnratio, _p(pts), C.byref(ntm), _p(match), C.byref(nm)), self._ctx.handle,
              "orbhip_search_local_points")
        return pts[:len(keys)].copy(), ntm.value, nm.value, match[:n].copy()
