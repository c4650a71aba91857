"""Independent model of the projection loops of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
(ref: src/ORBmatcher.cc:1366-1413) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ref: :1516-1558), written
from the cited lines: numpy with one rounding per stated operation (float64 sums and the float64 reciprocal, explicit float32
everywhere else) and the C library's own logf for the level -- not the threshold table the device uses.  The loops produce the
queries; the window search itself is the oracle's (orb_oracle_py.search_by_projection).

Stated divergences: a point with a non-finite position, reciprocal depth, u or v, with dist3D == 0 or not
finite, with a non-finite mfMaxDistance / dist3D, or with a key the store does not know is inactive."""
import numpy as np

from localmap_model import QUERY_DTYPE, Store, gemm3, predict_scale

f32, f64 = np.float32, np.float64
Q_ACTIVE, Q_OBSERVED = 1, 2
MP_OBSERVED, MP_BAD = 1, 2
SAME, FORWARD, BACKWARD = 0, 1, 2

# why a source feature gives no query, in the order the loops test (0 = active)
(ACTIVE, NO_POINT, UNKNOWN, BAD, FOUND, NONFINITE, BEHIND, LEFT, RIGHT, TOP, BOTTOM, NEAR, FAR) = range(13)
EXITS = ("active", "no point", "unknown", "bad", "found", "nonfinite", "behind", "left", "right", "top", "bottom", "near", "far")


def motion_of(cur_Rcw, cur_tcw, last_Rcw, last_tcw, mb, mono):
    """The current camera's centre in the last camera's frame decides (ref: :1351-1365); never for monocular input."""
    Ow = gemm3(np.asarray(cur_Rcw, f32).reshape(3, 3).T, np.asarray(cur_tcw, f32).reshape(1, 3), np.zeros(3, f32))
    twc = (-Ow.astype(f64)).astype(f32)    # -(R' t): the gemm with alpha = -1 rounds the negated double sum
    tlc = gemm3(last_Rcw, twc, last_tcw)[0]
    if not mono and tlc[2] > f32(mb):
        return FORWARD
    if not mono and -tlc[2] > f32(mb):
        return BACKWARD
    return SAME


def project(cam, P):
    """Camera point (one gemm), invz = float(1.0 / double(z)), u and v with every float operation rounded on its own, and the
    position in the image: 0 inside (edges included), else LEFT / RIGHT / TOP / BOTTOM, NONFINITE first."""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    min_x, max_x, min_y, max_y = (f32(v) for v in cam["bounds"])
    with np.errstate(all="ignore"):
        Pc = gemm3(cam["Rcw"], P, cam["tcw"])
        invz = (f64(1.0) / Pc[:, 2].astype(f64)).astype(f32)
        u = (fx * Pc[:, 0]) * invz + cx
        v = (fy * Pc[:, 1]) * invz + cy
    assert u.dtype == f32 and v.dtype == f32 and invz.dtype == f32
    where = np.zeros(len(P), np.int32)
    for i in range(len(P)):
        if not (np.isfinite(P[i]).all() and np.isfinite(invz[i]) and np.isfinite(u[i]) and np.isfinite(v[i])):
            where[i] = NONFINITE
        elif u[i] < min_x:
            where[i] = LEFT
        elif u[i] > max_x:
            where[i] = RIGHT
        elif v[i] < min_y:
            where[i] = TOP
        elif v[i] > max_y:
            where[i] = BOTTOM
    return u, v, invz, where


def last_frame_queries(store, cam, th, keys, last_kps, motion):
    """keys[i] = the point of LastFrame.mvpMapPoints[i] (0: NULL or mvbOutlier[i]).  Returns (queries, exit codes, qdesc)."""
    n = len(keys)
    sf = np.asarray(cam["scale_factors"], f32)
    mbf, th = f32(cam["mbf"]), f32(th)
    q = np.zeros(n, QUERY_DTYPE)
    code = np.zeros(n, np.int32)
    qdesc = np.zeros((n, 32), np.uint8)
    have = [i for i in range(n) if int(keys[i]) in store.pts]
    for i in range(n):
        if int(keys[i]) == 0:
            code[i] = NO_POINT
        elif int(keys[i]) not in store.pts:
            code[i] = UNKNOWN
    if not have:
        return q, code, qdesc
    pts = [store.pts[int(keys[i])] for i in have]
    u, v, invz, where = project(cam, np.stack([p[0] for p in pts]))
    for j, i in enumerate(have):       # (isBad() is not tested here, ref: :1370-1372)
        if where[j] == NONFINITE:
            code[i] = NONFINITE
        elif invz[j] < f32(0):
            code[i] = BEHIND           # ref: :1383
        elif where[j]:
            code[i] = where[j]
        else:
            o = int(last_kps["octave"][i])
            lo, hi = {SAME: (o - 1, o + 1), FORWARD: (o, -1), BACKWARD: (0, o)}[motion]
            xr = f32(u[j] - f32(mbf * invz[j]))
            q[i] = (u[j], v[j], f32(th * sf[o]), xr, lo, hi, last_kps["angle"][i], Q_ACTIVE | (Q_OBSERVED if pts[j][5] & MP_OBSERVED else 0))
            qdesc[i] = pts[j][4]
    return q, code, qdesc


def keyframe_queries(store, cam, th, row_keys, found_keys, kf_kps):
    """row_keys[i] = pKF->GetMapPointMatches()[i] as a key (0: NULL).  Returns (queries, exit codes, qdesc)."""
    n = len(row_keys)
    sf = np.asarray(cam["scale_factors"], f32)
    th = f32(th)
    found = set(int(k) for k in found_keys)
    q = np.zeros(n, QUERY_DTYPE)
    code = np.zeros(n, np.int32)
    qdesc = np.zeros((n, 32), np.uint8)
    have = []
    for i in range(n):
        k = int(row_keys[i])
        if k == 0:
            code[i] = NO_POINT
        elif k not in store.pts:
            code[i] = UNKNOWN
        elif store.pts[k][5] & MP_BAD:
            code[i] = BAD
        elif k in found:
            code[i] = FOUND
        else:
            have.append(i)
    if not have:
        return q, code, qdesc
    pts = [store.pts[int(row_keys[i])] for i in have]
    P = np.stack([p[0] for p in pts])
    u, v, invz, where = project(cam, P)
    Ow = np.asarray(cam["Ow"], f32).reshape(1, 3)
    with np.errstate(all="ignore"):
        PO = P - Ow
        sq = np.zeros(len(P), f64)
        for k in range(3):
            sq = sq + PO[:, k].astype(f64) * PO[:, k].astype(f64)
        dist = np.sqrt(sq).astype(f32)
        mn, mx = np.array([p[2] for p in pts], f32), np.array([p[3] for p in pts], f32)
        lo, hi = f32(0.8) * mn, f32(1.2) * mx
        ratio = mx / dist
    assert PO.dtype == f32 and lo.dtype == f32 and ratio.dtype == f32
    for j, i in enumerate(have):
        if where[j]:
            code[i] = where[j]                     # (no depth-sign test, ref: :1530-1539)
        elif not (dist[j] > 0 and np.isfinite(dist[j])):
            code[i] = NONFINITE
        elif dist[j] < lo[j]:
            code[i] = NEAR                         # ref: :1548
        elif dist[j] > hi[j]:
            code[i] = FAR
        elif not np.isfinite(ratio[j]):
            code[i] = NONFINITE
        else:
            lv = predict_scale(ratio[j], cam["log_scale_factor"], len(sf))
            q[i] = (u[j], v[j], f32(th * sf[lv]), 0.0, lv - 1, lv + 1, kf_kps["angle"][i], Q_ACTIVE | Q_OBSERVED)
            qdesc[i] = pts[j][4]
    return q, code, qdesc


def search_last_frame(oracle, store, cam, th, keys, last_kps, motion, kps, desc, gp, u_right=None, occupied=None, check_ori=True,
                      th_high=100):
    """Returns (queries, codes, qdesc, n_active, nmatches, match)."""
    q, code, qdesc = last_frame_queries(store, cam, th, keys, last_kps, motion)
    na = int((code == ACTIVE).sum())
    if len(kps) == 0 or len(keys) == 0:
        return q, code, qdesc, na, 0, np.full(len(kps), -1, np.int32)
    nm, match = oracle.search_by_projection(kps, desc, gp, q, qdesc, u_right=u_right, occupied=occupied, use_ratio=False,
                                            check_ori=check_ori, th_high=th_high)
    return q, code, qdesc, na, nm, match


def search_keyframe_points(oracle, store, cam, th, row_keys, found_keys, kf_kps, kps, desc, gp, occupied=None, check_ori=True,
                           th_high=100):
    q, code, qdesc = keyframe_queries(store, cam, th, row_keys, found_keys, kf_kps)
    na = int((code == ACTIVE).sum())
    if len(kps) == 0 or len(row_keys) == 0:
        return q, code, qdesc, na, 0, np.full(len(kps), -1, np.int32)
    nm, match = oracle.search_by_projection(kps, desc, gp, q, qdesc, u_right=None, occupied=occupied, use_ratio=False,
                                            check_ori=check_ori, th_high=th_high)
    return q, code, qdesc, na, nm, match


def claimed_twice(oracle, q, qdesc, kps, desc, gp, u_right=None, occupied=None, th_high=100):
    """How often a point took a feature that an earlier point of the same call held: the reference counts every assignment
    (nmatches++), so without the rotation check the return value exceeds the number of matched features by exactly that."""
    nm, match = oracle.search_by_projection(kps, desc, gp, q, qdesc, u_right=u_right, occupied=occupied, use_ratio=False,
                                            check_ori=False, th_high=th_high)
    return nm - int((match >= 0).sum())
