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
QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("proj_xr", "<f4"), ("min_level", "<i4"),
                        ("max_level", "<i4"), ("angle", "<f4"), ("flags", "<i4")])   # orbhip_proj_query
MOTION_SAME, MOTION_FORWARD, MOTION_BACKWARD = 0, 1, 2
FUSE_TARGET_DTYPE = np.dtype([("set_key", "<u8"), ("cam", CAMERA_DTYPE), ("inv_level_sigma2", "<f4", 16)], align=True)   # orbhip_fuse_target
REFRESH_DESC, REFRESH_NORMAL, KF_BAD = 1, 2, 1
REFRESH_KF_DTYPE = np.dtype([("set_key", "<u8"), ("Ow", "<f4", 3), ("flags", "<u4")])   # orbhip_refresh_kf
REFRESH_PARAMS_DTYPE = np.dtype([("scale_factors", "<f4", 16), ("nlevels", "<i4"), ("what", "<i4")])   # orbhip_refresh_params
SIM3D_DTYPE = np.dtype([("q", "<f8", 4), ("t", "<f8", 3), ("s", "<f8")])   # orbhip_sim3d: q = x y z w
CORRECT_XF_DTYPE = np.dtype([("Siw", SIM3D_DTYPE), ("corrected_Swi", SIM3D_DTYPE)])   # orbhip_correct_xf
CORRECT_KF_DTYPE = np.dtype([("Ow_before", "<f4", 3), ("Ow_after", "<f4", 3), ("rank", "<i4")])   # orbhip_correct_kf
CORRECT_SE3_DTYPE = np.dtype([("Rcw_before", "<f4", 9), ("tcw_before", "<f4", 3), ("Rwc", "<f4", 9), ("twc", "<f4", 3)])   # orbhip_correct_se3
POINT_DTYPE =np.dtype([("u", "<f4"), ("v", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
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


def fuse_target(set_key, cam, inv_level_sigma2):
    """One orbhip_fuse_target record: the target's resident set, its camera record (camera(); th = the th of Fuse) and
    KeyFrame::mvInvLevelSigma2."""
    t = np.zeros(1, FUSE_TARGET_DTYPE)
    t["set_key"], t["cam"] = set_key, np.ascontiguousarray(cam, CAMERA_DTYPE)[0]
    sg = np.asarray(inv_level_sigma2, f32)
    t["inv_level_sigma2"][0][:len(sg)] = sg
    return t


def level_byte(octave, stereo, far):
    """The level byte of one key-frame feature (orbhip_map_kf_levels): mvKeysUn[i].octave (0..15), mvuRight[i] >= 0,
    mvDepth[i] > mThDepth || mvDepth[i] < 0."""
    assert 0 <= int(octave) <= 15
    return int(octave) | (0x40 if stereo else 0) | (0x80 if far else 0)


def predict_scale_table(log_scale_factor, nlevels):
    """The threshold table of PredictScale (host only): T[k] = smallest float ratio whose level exceeds k."""
    t = np.zeros(max(nlevels - 1, 1), f32)
    check(capi.load().orbhip_debug_predict_scale_table(f32(log_scale_factor), nlevels, _p(t)), None,
          "orbhip_debug_predict_scale_table")
    return t[:nlevels - 1]


class LocalMap:
    """The map points of one context (an ORBextractor, or anything with .handle): put / update_flags / erase / clear / search."""

    def __init__(self, ctx, max_points, max_kfs=0, max_row=0):
        self._L = capi.load()
        self._ctx = ctx
        check(self._L.orbhip_map_init(ctx.handle, max_points), ctx.handle, "orbhip_map_init")
        if max_kfs:
            self.kf_init(max_kfs, max_row)

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

    # ---- the key-frame -> map-point table, the vote and the ordered union ----
    def kf_init(self, max_kfs, max_row):
        check(self._L.orbhip_map_kf_init(self._ctx.handle, max_kfs, max_row), self._ctx.handle, "orbhip_map_kf_init")

    def kf_clear(self):
        check(self._L.orbhip_map_kf_clear(self._ctx.handle), self._ctx.handle, "orbhip_map_kf_clear")

    def kf_info(self):
        """(live rows, max_kfs, max_row)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self._L.orbhip_map_kf_info(self._ctx.handle, C.byref(a), C.byref(b), C.byref(c)), self._ctx.handle, "orbhip_map_kf_info")
        return a.value, b.value, c.value

    def kf_put(self, kf_key, point_keys):
        pk = np.ascontiguousarray(point_keys, np.uint64)
        check(self._L.orbhip_map_kf_put(self._ctx.handle, kf_key, len(pk), _p(pk)), self._ctx.handle, "orbhip_map_kf_put")

    def kf_set(self, kf_key, idx, point_keys):
        idx, pk = np.ascontiguousarray(idx, np.int32).ravel(), np.ascontiguousarray(point_keys, np.uint64).ravel()
        assert len(idx) == len(pk)
        check(self._L.orbhip_map_kf_set(self._ctx.handle, kf_key, len(idx), _p(idx), _p(pk)), self._ctx.handle, "orbhip_map_kf_set")

    def kf_erase(self, kf_key):
        check(self._L.orbhip_map_kf_erase(self._ctx.handle, kf_key), self._ctx.handle, "orbhip_map_kf_erase")

    def vote(self, frame_point_keys, cap=None):
        """(kf_keys ascending, counts) of the key frames that hold at least one of the frame's points."""
        fk = np.ascontiguousarray(frame_point_keys, np.uint64)
        cap = self.kf_info()[1] if cap is None else cap
        keys, counts, n = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.int32), C.c_int()
        try:
            check(self._L.orbhip_map_vote(self._ctx.handle, len(fk), _p(fk), _p(keys), _p(counts), cap, C.byref(n)), self._ctx.handle,
                  "orbhip_map_vote")
        except capi.OrbHipError as e:     # too little room: the first cap entries are filled, .total has the number
            e.partial, e.total = (keys[:cap].copy(), counts[:cap].copy()), n.value
            raise
        return keys[:n.value].copy(), counts[:n.value].copy()

    def collect(self, kf_keys, cap):
        """The keys of mvpLocalMapPoints for mvpLocalKeyFrames = kf_keys, in the reference's order."""
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        out, n = np.zeros(max(cap, 1), np.uint64), C.c_int()
        try:
            check(self._L.orbhip_map_collect(self._ctx.handle, len(kk), _p(kk), _p(out), cap, C.byref(n)), self._ctx.handle,
                  "orbhip_map_collect")
        except capi.OrbHipError as e:
            e.partial, e.total = out[:cap].copy(), n.value
            raise
        return out[:n.value].copy()

    def covis(self, kf_keys, th=15, cap=None):
        """orbhip_map_covis: KeyFrame::UpdateConnections' counts and lists for every key frame of kf_keys.
        Returns one (keys, weights, ordered_keys) triple per query: the key frames that share a point with it in ascending key
        order with their weights (mConnectedKeyFrameWeights), and mvpOrderedConnectedKeyFrames as keys.  cap: room for the links of
        all queries together (default: queries times live key frames, which always suffices)."""
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        nq = len(kk)
        cap = nq * self.kf_info()[0] if cap is None else cap
        off, nord = np.full(nq + 1, -1, np.int32), np.full(max(nq, 1), -1, np.int32)
        nbr, w, order = np.zeros(max(cap, 1), np.uint64), np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1, np.int32)
        n = C.c_int(-1)
        try:
            check(self._L.orbhip_map_covis(self._ctx.handle, nq, _p(kk), th, _p(off), _p(nbr), _p(w), _p(order), _p(nord), cap,
                                           C.byref(n)), self._ctx.handle, "orbhip_map_covis")
        except capi.OrbHipError as e:     # too little room: .total has the number, .outputs what the call left in its outputs
            e.total, e.outputs = n.value, (off, nbr, w, order, nord)
            raise
        assert n.value == off[nq]
        out = []
        for q in range(nq):
            a, b = int(off[q]), int(off[q + 1])
            out.append((nbr[a:b].copy(), w[a:b].copy(), nbr[a:b][order[a:a + nord[q]]].copy()))
        return out

    # ---- the counts of KeyFrameCulling ----
    def kf_levels(self, kf_keys, rows_of_bytes, off=None):
        """orbhip_map_kf_levels: one level byte (level_byte()) per feature of every key frame of kf_keys, in one upload.  off: the
        offsets to pass instead of those of the rows' lengths (for the tests of the call's checks)."""
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        rows = [np.ascontiguousarray(r, np.uint8).ravel() for r in rows_of_bytes]
        assert len(rows) == len(kk)
        if off is None:
            off = np.zeros(len(kk) + 1, np.int32)
            off[1:] = np.cumsum([len(r) for r in rows])
        off = np.ascontiguousarray(off, np.int32)
        assert len(off) == len(kk) + 1
        b = np.concatenate(rows + [np.zeros(1, np.uint8)])
        check(self._L.orbhip_map_kf_levels(self._ctx.handle, len(kk), _p(kk), _p(off), _p(b)), self._ctx.handle, "orbhip_map_kf_levels")

    def kf_levels_missing(self):
        """The keys of the live rows whose levels are missing or shorter than the row, ascending."""
        cap = self.kf_info()[1]
        out, n = np.zeros(max(cap, 1), np.uint64), C.c_int()
        check(self._L.orbhip_map_kf_levels_missing(self._ctx.handle, _p(out), cap, C.byref(n)), self._ctx.handle,
              "orbhip_map_kf_levels_missing")
        return out[:n.value].copy()

    def cull(self, kf_keys, monocular, th_obs=3, want_entries=False):
        """orbhip_map_cull: (counts [K][2] = n_mps, n_redundant; redundant [K] bool) for the candidates kf_keys on the map as it is,
        and with want_entries entry_state [K][max_row] behind them.  The buffers start as -7 / 77 so that a caller sees what a failed
        call left alone (e.outputs)."""
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        K = len(kk)
        counts, red = np.full((max(K, 1), 2), -7, np.int32), np.full(max(K, 1), 77, np.uint8)
        st = np.full((max(K, 1), self.kf_info()[2]), 77, np.uint8) if want_entries else None
        try:
            check(self._L.orbhip_map_cull(self._ctx.handle, K, _p(kk), int(bool(monocular)), th_obs, _p(counts), _p(red), _p(st)),
                  self._ctx.handle, "orbhip_map_cull")
        except capi.OrbHipError as e:
            e.outputs = (counts, red, st)
            raise
        out = (counts[:K].copy(), red[:K].astype(bool))
        return out + (st[:K].copy(),) if want_entries else out

    # ---- the structure of local bundle adjustment's problem ----
    def ba_problem(self, kf_keys, cap_points, cap_edges, cap_fixed):
        """orbhip_map_ba_problem for the local key frames kf_keys: (point_keys, edge_off [npoints + 1], edges [nedges][2] = kf, idx,
        fixed_keys).  kf < len(kf_keys) names kf_keys[kf], otherwise fixed_keys[kf - len(kf_keys)].  The buffers start as 7 / -7 so
        that a caller sees what a failed call left alone (e.outputs); e.counts has the three counts as the call left them."""
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        pts, fixed = np.full(max(cap_points, 1), 7, np.uint64), np.full(max(cap_fixed, 1), 7, np.uint64)
        off, edges = np.full(max(cap_points, 0) + 1, -7, np.int32), np.full((max(cap_edges, 1), 2), -7, np.int32)
        n_p, n_e, n_f = C.c_int(-7), C.c_int(-7), C.c_int(-7)
        try:
            check(self._L.orbhip_map_ba_problem(self._ctx.handle, len(kk), _p(kk), _p(pts), cap_points, C.byref(n_p), _p(off), _p(edges),
                                                cap_edges, C.byref(n_e), _p(fixed), cap_fixed, C.byref(n_f)), self._ctx.handle,
                  "orbhip_map_ba_problem")
        except capi.OrbHipError as e:
            e.outputs, e.counts = (pts, off, edges, fixed), (n_p.value, n_e.value, n_f.value)
            raise
        return pts[:n_p.value].copy(), off[:n_p.value + 1].copy(), edges[:n_e.value].copy(), fixed[:n_f.value].copy()

    def search_by_bow_candidates(self, mode, fixed_set_key, fixed_row_key, n_fixed, candidates, th=50, nnratio=0.75, check_ori=True,
                                 gather=None, cap=None):
        """orbhip_search_by_bow_candidates: SearchByBoW of the fixed set of n_fixed features against K
        candidates, candidates = [(set_key, row_key), ...].  mode 0: SearchByBoW(pKF_k, F), mode 1: SearchByBoW(pCurrentKF, pKF_k).
        gather (mode 0): None, or (min_matches, level_sigma2, th2) for the PnPsolver arrays; cap: their room in entries (default
        K * n_fixed).  Returns (matches [K][n_fixed], nmatches [K]) and, with gather, a dict off / kp_idx / kf_idx / P3Dw / P2D /
        max_err behind them.  The buffers start as -7 so that a caller sees what a failed call left alone (e.outputs)."""
        cd = np.zeros(max(len(candidates), 1), capi.BOW_CANDIDATE_DTYPE)
        K = len(candidates)
        for k, (sk, rk) in enumerate(candidates):
            cd["set_key"][k], cd["row_key"][k] = sk, rk
        matches, nm = np.full(max(K * n_fixed, 1), -7, np.int32), np.full(max(K, 1), -7, np.int32)
        if gather is None:
            args = [0, None, 0, f32(0), None, None, None, None, None, None, 0, None]
            outs = (matches, nm)
        else:
            min_matches, sigma2, th2 = gather
            sigma2 = np.ascontiguousarray(sigma2, f32)
            cap = K * n_fixed if cap is None else cap
            m = max(cap, 1)
            off, kp, kf = np.full(K + 1, -7, np.int32), np.full(m, -7, np.int32), np.full(m, -7, np.int32)
            P3, P2, me = np.full((m, 3), -7, f32), np.full((m, 2), -7, f32), np.full(m, -7, f32)
            nt = C.c_int(-7)
            args = [min_matches, _p(sigma2), len(sigma2), f32(th2), _p(off), _p(kp), _p(kf), _p(P3), _p(P2), _p(me), cap, C.byref(nt)]
            outs = (matches, nm, off, kp, kf, P3, P2, me)
        try:
            check(self._L.orbhip_search_by_bow_candidates(self._ctx.handle, mode, fixed_set_key, fixed_row_key, _p(cd), K, th, f32(nnratio),
                                                          1 if check_ori else 0, _p(matches), _p(nm), *args), self._ctx.handle,
                  "orbhip_search_by_bow_candidates")
        except capi.OrbHipError as e:
            e.total, e.outputs = (None if gather is None else nt.value), outs
            raise
        res = (matches[:K * n_fixed].reshape(K, n_fixed).copy(), nm[:K].copy())
        if gather is None or K == 0:
            return res
        t = nt.value
        assert t == off[K]
        return res + ({"off": off.copy(), "kp_idx": kp[:t].copy(), "kf_idx": kf[:t].copy(), "P3Dw": P3[:t].copy(), "P2D": P2[:t].copy(),
                       "max_err": me[:t].copy()},)

    def track(self, frame_key, n, cam, kf_keys, seen_keys, cap, nnratio=0.8, u_right=None, occupied=None):
        """collect + search in one call.  Returns (local_keys, points, n_to_match, nmatches, match)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        kk, sk = np.ascontiguousarray(kf_keys, np.uint64), np.ascontiguousarray(seen_keys, np.uint64)
        ur = None if u_right is None else np.ascontiguousarray(u_right, f32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        keys, pts = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), POINT_DTYPE)
        match = np.empty(max(n, 1), np.int32)
        nl, ntm, nm = C.c_int(), C.c_int(), C.c_int()
        try:
            check(self._L.orbhip_track_local_points(self._ctx.handle, frame_key, _p(ur), _p(occ), _p(cam), len(kk), _p(kk), len(sk), _p(sk),
                                                    nnratio, _p(keys), cap, C.byref(nl), _p(pts), C.byref(ntm), _p(match), C.byref(nm)),
                  self._ctx.handle, "orbhip_track_local_points")
        except capi.OrbHipError as e:
            e.partial, e.total = keys[:cap].copy(), nl.value
            raise
        return keys[:nl.value].copy(), pts[:nl.value].copy(), ntm.value, nm.value, match[:n].copy()

    # ---- Tracking's other two guided searches on the resident map ----
    def search_last_frame(self, cur_key, n, last_key, last_point_keys, cam, motion=MOTION_SAME, u_right=None, occupied=None,
                          check_ori=True, th_high=100, want_queries=True):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) between two resident sets; cam["th"] is the th of the call.
        last_point_keys: the last frame's points as keys (0: none or an outlier).  Returns (queries or None, n_active, nmatches,
        match[n] indexing the last frame's features)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        lk = np.ascontiguousarray(last_point_keys, np.uint64)
        ur = None if u_right is None else np.ascontiguousarray(u_right, f32)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        q = np.zeros(max(len(lk), 1), QUERY_DTYPE) if want_queries else None
        match = np.empty(max(n, 1), np.int32)
        na, nm = C.c_int(), C.c_int()
        check(self._L.orbhip_search_last_frame(self._ctx.handle, cur_key, last_key, _p(lk), len(lk), _p(cam), motion, _p(ur), _p(occ),
                                               1 if check_ori else 0, th_high, _p(q), C.byref(na), _p(match), C.byref(nm)),
              self._ctx.handle, "orbhip_search_last_frame")
        return (None if q is None else q[:len(lk)].copy()), na.value, nm.value, match[:n].copy()

    def search_keyframe_points(self, cur_key, n, kf_set_key, kf_row_key, nrow, found_keys, cam, occupied=None, check_ori=True,
                               th_high=100, want_queries=True):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): the key frame's row of nrow entries against the
        resident set cur_key.  Returns (queries or None, n_active, nmatches, match[n] indexing the key frame's features)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        fk = np.ascontiguousarray(found_keys, np.uint64)
        occ = None if occupied is None else np.ascontiguousarray(occupied, np.uint8)
        q = np.zeros(max(nrow, 1), QUERY_DTYPE) if want_queries else None
        match = np.empty(max(n, 1), np.int32)
        na, nm = C.c_int(), C.c_int()
        check(self._L.orbhip_search_keyframe_points(self._ctx.handle, cur_key, kf_set_key, kf_row_key, _p(fk), len(fk), _p(cam), _p(occ),
                                                    1 if check_ori else 0, th_high, _p(q), C.byref(na), _p(match), C.byref(nm)),
              self._ctx.handle, "orbhip_search_keyframe_points")
        return (None if q is None else q[:nrow].copy()), na.value, nm.value, match[:n].copy()

    # ---- ORBmatcher::Fuse for LocalMapping::SearchInNeighbors on the resident map ----
    def fuse_row(self, src_row_key, n, targets, skip=None, u_right=None, want_queries=True):
        """The first pass: the n entries of key frame src_row_key's row into the K targets (fuse_targets).  skip: [K][n] or None;
        u_right: the targets' arrays one after the other, or None.  Returns (queries [K][n] or None, best_idx, best_dist, n_active [K])."""
        t = np.ascontiguousarray(targets, FUSE_TARGET_DTYPE)
        K = len(t)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, n)
        ur = None if u_right is None else np.ascontiguousarray(u_right, f32)
        q = np.zeros(max(K * n, 1), QUERY_DTYPE) if want_queries else None
        bi, bd = np.empty(max(K * n, 1), np.int32), np.empty(max(K * n, 1), np.int32)
        na = np.zeros(max(K, 1), np.int32)
        check(self._L.orbhip_fuse_row(self._ctx.handle, src_row_key, _p(t), K, _p(sk), _p(ur), _p(q), _p(bi), _p(bd), _p(na)),
              self._ctx.handle, "orbhip_fuse_row")
        return (None if q is None else q[:K * n].reshape(K, n).copy()), bi[:K * n].reshape(K, n).copy(), bd[:K * n].reshape(K, n).copy(), na[:K].copy()

    def fuse_collect(self, target, cur_row_key, kf_keys, cap, u_right=None, want_queries=True):
        """The second pass: the ordered union of the rows kf_keys into the one target, whose own row is cur_row_key.  Returns
        (keys, queries or None, best_idx, best_dist, n_active)."""
        t = np.ascontiguousarray(target, FUSE_TARGET_DTYPE)
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        ur = None if u_right is None else np.ascontiguousarray(u_right, f32)
        keys = np.zeros(max(cap, 1), np.uint64)
        q = np.zeros(max(cap, 1), QUERY_DTYPE) if want_queries else None
        bi, bd = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32)
        nc, na = C.c_int(), C.c_int()
        try:
            check(self._L.orbhip_fuse_collect(self._ctx.handle, _p(t), cur_row_key, len(kk), _p(kk), _p(ur), _p(keys), cap, C.byref(nc),
                                              _p(q), _p(bi), _p(bd), C.byref(na)), self._ctx.handle, "orbhip_fuse_collect")
        except capi.OrbHipError as e:
            e.partial, e.total = keys[:cap].copy(), nc.value
            raise
        m = nc.value
        return keys[:m].copy(), (None if q is None else q[:m].copy()), bi[:m].copy(), bd[:m].copy(), na.value

    # ---- LoopClosing's projection searches on the resident map ----
    def kf_set_batch(self, kf_keys, idx, point_keys):
        """kf_set for entries of many key frames in one call: entry j sets index idx[j] of key frame kf_keys[j]'s row."""
        kk = np.ascontiguousarray(kf_keys, np.uint64).ravel()
        idx, pk = np.ascontiguousarray(idx, np.int32).ravel(), np.ascontiguousarray(point_keys, np.uint64).ravel()
        assert len(kk) == len(idx) == len(pk)
        check(self._L.orbhip_map_kf_set_batch(self._ctx.handle, len(kk), _p(kk), _p(idx), _p(pk)), self._ctx.handle,
              "orbhip_map_kf_set_batch")

    def fuse_sim3(self, targets, target_row_keys, point_keys, want_queries=True):
        """Fuse(pKF, Scw, vpPoints, th, ...) up to the map edits, for K targets (fuse_target records whose cam holds the decomposed
        similarity) in one call.  target_row_keys: [K] (0: none) or None.  Returns (queries [K][n] or None, best_idx, best_dist,
        n_active [K])."""
        t = np.ascontiguousarray(targets, FUSE_TARGET_DTYPE)
        pk = np.ascontiguousarray(point_keys, np.uint64).ravel()
        K, n = len(t), len(pk)
        rk = None if target_row_keys is None else np.ascontiguousarray(target_row_keys, np.uint64).ravel()
        assert rk is None or len(rk) == K
        q = np.zeros(max(K * n, 1), QUERY_DTYPE) if want_queries else None
        bi, bd = np.empty(max(K * n, 1), np.int32), np.empty(max(K * n, 1), np.int32)
        na = np.zeros(max(K, 1), np.int32)
        check(self._L.orbhip_fuse_sim3(self._ctx.handle, _p(t), _p(rk), K, _p(pk), n, _p(q), _p(bi), _p(bd), _p(na)), self._ctx.handle,
              "orbhip_fuse_sim3")
        return (None if q is None else q[:K * n].reshape(K, n).copy()), bi[:K * n].reshape(K, n).copy(), bd[:K * n].reshape(K, n).copy(), na[:K].copy()

    def search_loop_points(self, target, n, kf_keys, matched_keys, cap, th_high=50, want_queries=True):
        """ComputeSim3's union of the rows kf_keys and SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) over it; n = the size of
        the target's set, matched_keys: [n] (0: NULL) or None.  Returns (keys, queries or None, n_active, nmatches, match [n]
        indexing keys)."""
        t = np.ascontiguousarray(target, FUSE_TARGET_DTYPE)
        kk = np.ascontiguousarray(kf_keys, np.uint64)
        mk = None if matched_keys is None else np.ascontiguousarray(matched_keys, np.uint64).ravel()
        assert mk is None or len(mk) == n
        keys = np.zeros(max(cap, 1), np.uint64)
        q = np.zeros(max(cap, 1), QUERY_DTYPE) if want_queries else None
        match = np.empty(max(n, 1), np.int32)
        npts, na, nm = C.c_int(), C.c_int(), C.c_int()
        try:
            check(self._L.orbhip_search_loop_points(self._ctx.handle, _p(t), len(kk), _p(kk), _p(mk), th_high, _p(keys), cap, C.byref(npts),
                                                    _p(q), C.byref(na), _p(match), C.byref(nm)), self._ctx.handle,
                  "orbhip_search_loop_points")
        except capi.OrbHipError as e:
            e.partial, e.total = keys[:cap].copy(), npts.value
            raise
        m = npts.value
        return keys[:m].copy(), (None if q is None else q[:m].copy()), na.value, nm.value, match[:n].copy()

    # ---- ORBmatcher::SearchBySim3 on the resident map ----
    def search_by_sim3(self, sides, row_keys, n1, n2, sR21, t21, sR12, t12, th, th_high=100, taken1=None, taken2=None, want=True):
        """orbhip_search_by_sim3.  sides: two fuse_target records (side 1, side 2; cam = the key frame's own pose), row_keys [2],
        n1 / n2 = the lengths of the two rows (= the sets' feature counts), the similarity composed by the caller, taken1 [n1] /
        taken2 [n2] bytes or None.  Returns (match12 [n1], nfound, n_active [2], (queries1, best1, dist1), (queries2, best2,
        dist2)); with want=False the optional outputs are passed as NULL and the two tuples come back None."""
        t = np.ascontiguousarray(sides, FUSE_TARGET_DTYPE).ravel()
        rk = np.ascontiguousarray(row_keys, np.uint64).ravel()
        assert len(t) == 2 and len(rk) == 2
        sim = [np.ascontiguousarray(a, f32).ravel() for a in (sR21, t21, sR12, t12)]
        assert [len(a) for a in sim] == [9, 3, 9, 3]
        tk1 = None if taken1 is None else np.ascontiguousarray(taken1, np.uint8).ravel()
        tk2 = None if taken2 is None else np.ascontiguousarray(taken2, np.uint8).ravel()
        assert (tk1 is None or len(tk1) == n1) and (tk2 is None or len(tk2) == n2)
        match = np.empty(max(n1, 1), np.int32)
        nf, na = C.c_int(), np.zeros(2, np.int32)
        opt = [None] * 6
        if want:
            opt = [a for n in (n1, n2) for a in (np.zeros(max(n, 1), QUERY_DTYPE), np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32))]
        check(self._L.orbhip_search_by_sim3(self._ctx.handle, _p(t), _p(rk), _p(sim[0]), _p(sim[1]), _p(sim[2]), _p(sim[3]), C.c_float(th),
                                            th_high, _p(tk1), _p(tk2), _p(match), C.byref(nf), _p(na), *[_p(a) for a in opt]),
              self._ctx.handle, "orbhip_search_by_sim3")
        if not want:
            return match[:n1].copy(), nf.value, na.copy(), None, None
        return (match[:n1].copy(), nf.value, na.copy(), tuple(a[:n1].copy() for a in opt[:3]), tuple(a[:n2].copy() for a in opt[3:]))

    # ---- map points refreshed in place: descriptor, normal, depth ----
    def map_refresh(self, scale_factors, nlevels, what, kfs, point_keys, off, obs_kf, obs_idx, ref_pos, want=True):
        """orbhip_map_refresh.  kfs: REFRESH_KF_DTYPE records; the lists as CSR (off [P + 1], obs_kf / obs_idx [off[P]]) in ascending
        KeyFrame::mnId; ref_pos [P].  Returns (status, best_pos, desc, normal, min_dist, max_dist); with want=False every output but
        status is passed as NULL and comes back None."""
        prm = np.zeros(1, REFRESH_PARAMS_DTYPE)
        sf = np.asarray(scale_factors, f32)
        prm["scale_factors"][0][:len(sf)] = sf[:16]
        prm["nlevels"], prm["what"] = nlevels, what
        kfs = np.ascontiguousarray(kfs, REFRESH_KF_DTYPE)
        pk = np.ascontiguousarray(point_keys, np.uint64).ravel()
        off = np.ascontiguousarray(off, np.int32).ravel()
        ok, oi = np.ascontiguousarray(obs_kf, np.int32).ravel(), np.ascontiguousarray(obs_idx, np.int32).ravel()
        rp = np.ascontiguousarray(ref_pos, np.int32).ravel()
        P = len(pk)
        assert len(off) == P + 1 and len(rp) == P and len(ok) == len(oi)
        m = max(P, 1)
        status = np.zeros(m, np.uint8)
        outs = [np.zeros(m, np.int32), np.zeros((m, 32), np.uint8), np.zeros((m, 3), f32), np.zeros(m, f32), np.zeros(m, f32)] if want else [None] * 5
        check(self._L.orbhip_map_refresh(self._ctx.handle, _p(prm), len(kfs), _p(kfs), P, _p(pk), _p(off), _p(ok), _p(oi), _p(rp), _p(status),
                                         *[_p(x) for x in outs]), self._ctx.handle, "orbhip_map_refresh")
        return (status[:P].copy(),) + tuple(None if x is None else x[:P].copy() for x in outs)

    def map_get(self, keys, want=("pos", "normal", "min_dist", "max_dist", "desc", "flags")):
        """orbhip_map_get: the store's entries for keys, as a dict of the outputs named in want (the others are passed as NULL)."""
        keys = np.ascontiguousarray(keys, np.uint64).ravel()
        n, m = len(keys), max(len(keys), 1)
        bufs = {"pos": np.zeros((m, 3), f32), "normal": np.zeros((m, 3), f32), "min_dist": np.zeros(m, f32), "max_dist": np.zeros(m, f32),
                "desc": np.zeros((m, 32), np.uint8), "flags": np.zeros(m, np.uint8)}
        args = [_p(bufs[k]) if k in want else None for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags")]
        check(self._L.orbhip_map_get(self._ctx.handle, n, _p(keys), *args), self._ctx.handle, "orbhip_map_get")
        return {k: bufs[k][:n].copy() for k in want}

    # ---- map points moved in place: CorrectLoop's Sim3 pass and the global-BA update ----
    def map_correct_sim3(self, scale_factors, nlevels, xf, kfs, point_keys, corr, off, obs_kf, ref_pos, ref_level, want=True):
        """orbhip_map_correct_sim3.  xf: CORRECT_XF_DTYPE records in the loop's order; kfs: CORRECT_KF_DTYPE records; corr [P]; the lists
        as CSR (off [P + 1], obs_kf [off[P]]) in ascending KeyFrame::mnId; ref_pos, ref_level [P].  Returns (status, pos, normal,
        min_dist, max_dist); with want=False every output but status is passed as NULL and comes back None."""
        prm = np.zeros(1, REFRESH_PARAMS_DTYPE)
        sf = np.asarray(scale_factors, f32)
        prm["scale_factors"][0][:len(sf)] = sf[:16]
        prm["nlevels"] = nlevels
        xf = np.ascontiguousarray(xf, CORRECT_XF_DTYPE)
        kfs = np.ascontiguousarray(kfs, CORRECT_KF_DTYPE)
        pk = np.ascontiguousarray(point_keys, np.uint64).ravel()
        co, off = np.ascontiguousarray(corr, np.int32).ravel(), np.ascontiguousarray(off, np.int32).ravel()
        ok, rp = np.ascontiguousarray(obs_kf, np.int32).ravel(), np.ascontiguousarray(ref_pos, np.int32).ravel()
        rl = np.ascontiguousarray(ref_level, np.uint8).ravel()
        P = len(pk)
        assert len(off) == P + 1 and len(rp) == P and len(co) == P and len(rl) == P
        m = max(P, 1)
        status = np.zeros(m, np.uint8)
        outs = [np.zeros((m, 3), f32), np.zeros((m, 3), f32), np.zeros(m, f32), np.zeros(m, f32)] if want else [None] * 4
        check(self._L.orbhip_map_correct_sim3(self._ctx.handle, _p(prm), len(xf), _p(xf), len(kfs), _p(kfs), P, _p(pk), _p(co), _p(off), _p(ok),
                                              _p(rp), _p(rl), _p(status), *[_p(x) for x in outs]), self._ctx.handle, "orbhip_map_correct_sim3")
        return (status[:P].copy(),) + tuple(None if x is None else x[:P].copy() for x in outs)

    def map_correct_se3(self, xf, point_keys, corr, pos_set=None, want=True):
        """orbhip_map_correct_se3.  xf: CORRECT_SE3_DTYPE records; corr [P] in [0, K) or -1 = take pos_set [P][3].  Returns (status, pos)."""
        xf = np.ascontiguousarray(xf, CORRECT_SE3_DTYPE)
        pk = np.ascontiguousarray(point_keys, np.uint64).ravel()
        co = np.ascontiguousarray(corr, np.int32).ravel()
        ps = None if pos_set is None else np.ascontiguousarray(pos_set, f32).reshape(-1, 3)
        P = len(pk)
        assert len(co) == P and (ps is None or len(ps) == P)
        m = max(P, 1)
        status = np.zeros(m, np.uint8)
        pos = np.zeros((m, 3), f32) if want else None
        check(self._L.orbhip_map_correct_se3(self._ctx.handle, len(xf), _p(xf), P, _p(pk), _p(co), _p(ps), _p(status), _p(pos)),
              self._ctx.handle, "orbhip_map_correct_se3")
        return status[:P].copy(), (None if pos is None else pos[:P].copy())

    def search_last_frame_device(self, d_kps, d_desc, d_counts, cap, B, d_u_right, d_occupied, gp, d_cell_off, d_cell_idx, d_cam, d_slots,
                                 d_last_kps, d_motion, d_nq, cap_q, check_ori, th_high, d_queries, d_n_active, d_match, d_nmatches):
        """The batched, asynchronous form: every d_* is a device address (int; 0 where the header allows NULL); gp = (min_x,
        min_y, inv_w, inv_h).  Layouts as in include/orbhip.h.  No synchronisation."""
        check(self._L.orbhip_search_last_frame_device(self._ctx.handle, d_kps, d_desc, d_counts, cap, B, d_u_right or None,
                                                      d_occupied or None, gp[0], gp[1], gp[2], gp[3], d_cell_off, d_cell_idx, d_cam,
                                                      d_slots, d_last_kps, d_motion, d_nq, cap_q, 1 if check_ori else 0, th_high,
                                                      d_queries or None, d_n_active, d_match, d_nmatches), self._ctx.handle,
              "orbhip_search_last_frame_device")
