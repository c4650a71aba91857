"""Independent model of Frame::isInFrustum + MapPoint::PredictScale + the window of ORBmatcher::SearchByProjection(Frame&,
vector<MapPoint*>&, th) (ref: src/Frame.cc:613-669, src/MapPoint.cc:388-432, src/ORBmatcher.cc:45-137), written from the
definition in DESIGN.md section 10: numpy with one rounding per stated operation (float64 sums, explicit float32 casts) and the C
library's own logf for the level -- not the threshold table the device uses.  The window search itself is the oracle's
(orb_oracle_py.search_by_projection), fed with the queries built here."""
import ctypes as C
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]

# why a point is not in view, in the order isInFrustum tests (0 = in view)
IN_VIEW, BEHIND, LEFT, RIGHT, TOP, BOTTOM, NEAR, FAR, VIEWCOS, NOT_TESTED = range(10)
EXITS = ("in view", "behind", "left", "right", "top", "bottom", "near", "far", "viewcos", "not tested")

QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("proj_xr", "<f4"), ("min_level", "<i4"),
                        ("max_level", "<i4"), ("angle", "<f4"), ("flags", "<i4")])
POINT_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"), ("in_view", "<i4")])


def logf(x):
    return f32(_libm.logf(C.c_float(float(x))))


def predict_scale(ratio, log_scale_factor, nlevels):
    """ceil(logf(ratio) / mfLogScaleFactor) clamped to [0, nlevels - 1] (src/MapPoint.cc:417-432)."""
    x = logf(f32(ratio)) / f32(log_scale_factor)
    n = int(np.ceil(x))
    return 0 if n < 0 else (nlevels - 1 if n >= nlevels else n)


def gemm3(R, P, t):
    """R * P + t as OpenCV's float gemm: products and sums in double, one rounding to float per component."""
    R, P, t = np.asarray(R, f32).reshape(3, 3), np.asarray(P, f32).reshape(-1, 3), np.asarray(t, f32).reshape(3)
    out = np.empty(P.shape, f32)
    for r in range(3):
        s = np.zeros(len(P), f64)
        for k in range(3):
            s = s + f64(R[r, k]) * P[:, k].astype(f64)
        out[:, r] = (s + f64(t[r])).astype(f32)
    return out


def frustum(cam, pos, normal, min_dist, max_dist):
    """isInFrustum for every point.  cam: dict with Rcw, tcw, Ow, fx, fy, cx, cy, mbf, bounds (min_x, max_x, min_y, max_y),
    scale_factors, log_scale_factor, viewing_cos_limit.  Returns (records POINT_DTYPE, exit code per point)."""
    P = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    Pn = np.ascontiguousarray(normal, f32).reshape(-1, 3)
    mn, mx = np.asarray(min_dist, f32), np.asarray(max_dist, f32)
    n = len(P)
    fx, fy, cx, cy, mbf = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    min_x, max_x, min_y, max_y = (f32(v) for v in cam["bounds"])
    nlevels = len(cam["scale_factors"])
    rec = np.zeros(n, POINT_DTYPE)
    code = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        Pc = gemm3(cam["Rcw"], P, cam["tcw"])
        invz = f32(1.0) / Pc[:, 2]
        u = (fx * Pc[:, 0]) * invz + cx
        v = (fy * Pc[:, 1]) * invz + cy
        PO = P - np.asarray(cam["Ow"], f32).reshape(1, 3)
        sq = np.zeros(n, f64)
        dot = np.zeros(n, f64)
        for k in range(3):
            sq = sq + PO[:, k].astype(f64) * PO[:, k].astype(f64)
            dot = dot + PO[:, k].astype(f64) * Pn[:, k].astype(f64)
        dist = np.sqrt(sq).astype(f32)
        view = (dot / dist.astype(f64)).astype(f32)
        ratio = mx / dist
        xr = u - mbf * invz
        lo, hi = f32(0.8) * mn, f32(1.2) * mx
    assert u.dtype == f32 and xr.dtype == f32 and ratio.dtype == f32 and lo.dtype == f32
    limit = f32(cam["viewing_cos_limit"])
    for i in range(n):
        if Pc[i, 2] < f32(0.0):
            code[i] = BEHIND
        elif u[i] < min_x:
            code[i] = LEFT
        elif u[i] > max_x:
            code[i] = RIGHT
        elif v[i] < min_y:
            code[i] = TOP
        elif v[i] > max_y:
            code[i] = BOTTOM
        elif dist[i] < lo[i]:
            code[i] = NEAR
        elif dist[i] > hi[i]:
            code[i] = FAR
        elif view[i] < limit:
            code[i] = VIEWCOS
        else:
            rec[i] = (u[i], v[i], xr[i], view[i], predict_scale(ratio[i], cam["log_scale_factor"], nlevels), 1)
    return rec, code


def radius(view_cos, th):
    """RadiusByViewingCos (0.998 is a double compared with a float), times th when th != 1.0 (src/ORBmatcher.cc:61-66, 131-137)."""
    r = f32(2.5) if f64(f32(view_cos)) > 0.998 else f32(4.0)
    if float(f32(th)) != 1.0:
        r = f32(r * f32(th))
    return r


def queries(rec, observed, th, scale_factors):
    sf = np.asarray(scale_factors, f32)
    q = np.zeros(len(rec), QUERY_DTYPE)
    for i in np.nonzero(rec["in_view"])[0]:
        lv = int(rec["level"][i])
        q[i] = (rec["u"][i], rec["v"][i], f32(radius(rec["view_cos"][i], th) * sf[lv]), rec["proj_xr"][i], lv - 1, lv, 0.0,
                1 | (2 if observed[i] else 0))
    return q


class Store:
    """The store as a dictionary: key -> (pos, normal, min, max, desc, flags)."""

    def __init__(self, max_points):
        self.max_points, self.pts = max_points, {}

    def put(self, keys, pos, normal, mn, mx, desc, flags):
        new = {int(k) for k in keys} - set(self.pts)
        if len(self.pts) + len(new) > self.max_points:
            raise OverflowError
        for i, k in enumerate(keys):
            self.pts[int(k)] = [np.array(pos[i], f32), np.array(normal[i], f32), f32(mn[i]), f32(mx[i]), np.array(desc[i], np.uint8),
                                int(flags[i])]

    def update_flags(self, keys, flags):
        for k, f in zip(keys, flags):
            self.pts[int(k)][5] = int(f)

    def erase(self, keys):
        for k in keys:
            self.pts.pop(int(k), None)


def search_local_points(oracle, store, cam, th, keys, skip, kps, desc, gp, nnratio=0.8, u_right=None, occupied=None):
    """The second loop of Tracking::SearchLocalPoints + SearchByProjection.  Returns (records, exit codes, n_to_match, nmatches,
    match, queries, qdesc); kps None = a frame without features."""
    nq = len(keys)
    tested = np.array([(not skip[i]) and int(keys[i]) in store.pts and not (store.pts[int(keys[i])][5] & 2) for i in range(nq)], bool)
    rec = np.zeros(nq, POINT_DTYPE)
    code = np.full(nq, NOT_TESTED, np.int32)
    observed = np.zeros(nq, bool)
    qdesc = np.zeros((nq, 32), np.uint8)
    idx = np.nonzero(tested)[0]
    if len(idx):
        p = [store.pts[int(keys[i])] for i in idx]
        r, c = frustum(cam, np.stack([x[0] for x in p]), np.stack([x[1] for x in p]), np.array([x[2] for x in p], f32),
                       np.array([x[3] for x in p], f32))
        rec[idx], code[idx] = r, c
        observed[idx] = [bool(x[5] & 1) for x in p]
        qdesc[idx] = np.stack([x[4] for x in p])
    q = queries(rec, observed, th, cam["scale_factors"])
    ntm = int(rec["in_view"].sum())
    if kps is None or len(kps) == 0 or nq == 0:
        return rec, code, ntm, 0, np.zeros(0, np.int32), q, qdesc
    nm, match = oracle.search_by_projection(kps, desc, gp, q, qdesc, u_right=u_right, occupied=occupied, use_ratio=True,
                                            nnratio=nnratio, check_ori=False, th_high=100)
    return rec, code, ntm, nm, match, q, qdesc
