"""Independent model of ORBmatcher::SearchBySim3 (ref: src/ORBmatcher.cc:1102-1326), written from the cited lines: numpy with one
rounding per stated operation (float64 sums, explicit float32 everywhere else) and the C library's own logf for the level -- not the
threshold table the device uses.  It reads observation-free rows (a key frame's mvpMapPoints as keys, 0 = NULL) and the model store
of tests/localmap_model.py; the window search goes through the oracle exactly as tests/loopfuse_model.py does it.

What is particular to this search, against Fuse (tests/fuse_model.py): the camera point is two gemms, p = Rsw Xw + tsw rounded to
float and then sR p + t (:1159-1160, :1239-1240); dist3D is cv::norm of that camera point (:1179, :1259), not of P - Ow; there is no
viewing-angle test; fx, fy, cx, cy are key frame 1's in BOTH directions (:1105-1108, :1170, :1250) while IsInImage, PredictScale,
mvScaleFactors and the grid are the destination's; the bound on the best distance is TH_HIGH (:1221, :1301) and a pair counts only
when the two directions name each other (:1310-1323).

`variant` names one deliberate mistake (tests/test_sim3search_model.py shows that each changes at least one scene):
z_le, closed_bounds, other_assoc, norm_ow, dst_intrinsics, view_test, levels_plus, th_low, lt_th_high, no_agreement, one_direction,
ignore_taken2, stale_resolved.

Stated divergences: dist3D == 0 or not finite, a non-finite mfMaxDistance / dist3D and an entry the store
does not know are inactive."""
import numpy as np

import loopfuse_model as LM
from fuse_model import (ACTIVE, BAD, BEHIND, BOTTOM, EXITS, FAR, LEFT, MP_BAD, NEAR, NO_POINT, NONFINITE, Q_ACTIVE, Q_OBSERVED, RIGHT,   # noqa: F401
                        SKIPPED, TOP, UNKNOWN, VIEW, tally)
from localmap_model import QUERY_DTYPE, Store, gemm3, predict_scale   # noqa: F401

f32, f64 = np.float32, np.float64
TH_HIGH, TH_LOW = 100, 50
VARIANTS = ("z_le", "closed_bounds", "other_assoc", "norm_ow", "dst_intrinsics", "view_test", "levels_plus", "th_low", "lt_th_high",
            "no_agreement", "one_direction", "ignore_taken2", "stale_resolved")


def compose(s12, R12, t12):
    """(sR12, sR21, t21) of :1119-1121: s12 * R12 and (1.0 / s12) * R12.t() are the double factor times the float entry, rounded
    once; t21 = -sR21 * t12 is one gemm with alpha = -1 (double sum, one rounding)."""
    R12, t12 = np.asarray(R12, f32).reshape(3, 3), np.asarray(t12, f32).reshape(3)
    sR12 = (f64(f32(s12)) * R12.astype(f64)).astype(f32)
    sR21 = ((f64(1.0) / f64(f32(s12))) * R12.T.astype(f64)).astype(f32)
    t21 = np.zeros(3, f32)
    for r in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(sR21[r, k]) * f64(t12[k])
        t21[r] = f32(f64(-1.0) * s + f64(0.0))
    return sR12, sR21, t21


def direction_queries(store, src, sR, t, K1, dst, th, row, taken, variant=None, reused=None):
    """One projection loop (:1148-1192 / :1228-1272) over `row` (keys, 0 = NULL).  src: the source key frame's camera (Rcw, tcw);
    sR, t: the similarity into the destination camera; K1: key frame 1's camera (the intrinsics); dst: the destination's (bounds,
    scale tables; Ow only for the wrong variants).  Returns (queries, exit codes, qdesc)."""
    n = len(row)
    K = dst if variant == "dst_intrinsics" else K1
    fx, fy, cx, cy = (f32(K[k]) for k in ("fx", "fy", "cx", "cy"))
    sf = np.asarray(dst["scale_factors"], f32)
    min_x, max_x, min_y, max_y = (f32(b) for b in dst["bounds"])
    th = f32(th)
    q = np.zeros(n, QUERY_DTYPE)
    code = np.zeros(n, np.int32)
    qdesc = np.zeros((n, 32), np.uint8)
    for i in range(n):
        k = int(row[i])
        if k and k not in store.pts and variant == "stale_resolved" and reused and k in reused:
            k = int(reused[k])                     # the entry's slot went to another point: a resolver without generations takes it
        if k == 0:
            code[i] = NO_POINT                     # :1152
            continue
        if k not in store.pts:
            code[i] = UNKNOWN
            continue
        if taken is not None and taken[i]:
            code[i] = SKIPPED                      # :1152 vbAlreadyMatched
            continue
        P, Pn, mn, mx, d, fl = store.pts[k]
        if fl & MP_BAD:
            code[i] = BAD                          # :1155
            continue
        with np.errstate(all="ignore"):
            p1 = gemm3(src["Rcw"], P, src["tcw"])  # :1159
            p2 = gemm3(sR, p1, t)[0]               # :1160
            z = p2[2]
            invz = f32(1.0) / z                    # :1166
            if variant == "other_assoc":
                u, v = f32(f32(f32(fx * p2[0]) * invz) + cx), f32(f32(f32(fy * p2[1]) * invz) + cy)
            else:
                x, y = f32(p2[0] * invz), f32(p2[1] * invz)
                u, v = f32(f32(fx * x) + cx), f32(f32(fy * y) + cy)            # :1170-1171
            if variant == "norm_ow" or variant == "view_test":
                po = (np.asarray(P, f32) - np.asarray(dst["Ow"], f32)).astype(f32)
            vec = po if variant == "norm_ow" else p2
            sq = f64(0)
            for c in range(3):
                sq = sq + f64(vec[c]) * f64(vec[c])
            dist = f32(np.sqrt(sq))                # :1179 cv::norm(p3Dc2)
            lo, hi = f32(f32(0.8) * f32(mn)), f32(f32(1.2) * f32(mx))
            ratio = f32(f32(mx) / dist)
        behind = z <= f32(0.0) if variant == "z_le" else z < f32(0.0)
        right = u > max_x if variant == "closed_bounds" else u >= max_x
        bottom = v > max_y if variant == "closed_bounds" else v >= max_y
        if behind:
            code[i] = BEHIND                       # :1163
        elif u < min_x:
            code[i] = LEFT                         # :1174, KeyFrame::IsInImage
        elif right:
            code[i] = RIGHT
        elif v < min_y:
            code[i] = TOP
        elif bottom:
            code[i] = BOTTOM
        elif not (u >= min_x and v >= min_y and np.isfinite(u) and np.isfinite(v)):
            code[i] = NONFINITE                    # NaN fails IsInImage
        elif not (dist > 0 and np.isfinite(dist)):
            code[i] = NONFINITE                    # divergence
        elif dist < lo:
            code[i] = NEAR                         # :1182
        elif dist > hi:
            code[i] = FAR
        elif variant == "view_test" and sum(f64(po[c]) * f64(Pn[c]) for c in range(3)) < f64(0.5) * f64(dist):
            code[i] = VIEW
        elif not np.isfinite(ratio):
            code[i] = NONFINITE                    # divergence
        else:
            lv = predict_scale(ratio, dst["log_scale_factor"], len(sf))        # :1186
            q[i] = (u, v, f32(th * sf[lv]), 0.0, lv - 1, lv + 1 if variant == "levels_plus" else lv, 0.0, Q_ACTIVE | Q_OBSERVED)
            qdesc[i] = d
    return q, code, qdesc


def agree(best1, dist1, best2, dist2, th_high=TH_HIGH, variant=None):
    """:1221, :1301, :1310-1323.  Returns (match12, nfound)."""
    if variant == "th_low":
        th_high = TH_LOW
    keep = (lambda d: d < th_high) if variant == "lt_th_high" else (lambda d: d <= th_high)
    vn1 = np.where(keep(np.asarray(dist1)), best1, -1).astype(np.int32)
    vn2 = np.where(keep(np.asarray(dist2)), best2, -1).astype(np.int32)
    match = np.full(len(vn1), -1, np.int32)
    if variant == "no_agreement":
        match = vn1.copy()
    elif variant == "one_direction":
        for i2 in range(len(vn2)):
            if vn2[i2] >= 0:
                match[vn2[i2]] = i2
    else:
        for i1 in range(len(vn1)):
            i2 = int(vn1[i1])
            if i2 >= 0 and int(vn2[i2]) == i1:
                match[i1] = i2
    return match, int((match >= 0).sum())


def search_by_sim3(oracle, store, sides, rows, s12, R12, t12, th, th_high=TH_HIGH, taken1=None, taken2=None, variant=None, reused=None):
    """sides: two dicts(cam, kps, desc, gp); rows: the two key frames' mvpMapPoints as keys.  Returns a dict: q, code, qdesc, best,
    dist (each a pair: direction 0 = row 1 into key frame 2, direction 1 = row 2 into key frame 1), n_active, match12, nfound and the
    composed similarity (sR21, t21, sR12, t12)."""
    sR12, sR21, t21 = compose(s12, R12, t12)
    t12 = np.asarray(t12, f32).reshape(3)
    cam1, cam2 = sides[0]["cam"], sides[1]["cam"]
    if variant == "ignore_taken2":
        taken2 = None
    q1, c1, d1 = direction_queries(store, cam1, sR21, t21, cam1, cam2, th, rows[0], taken1, variant, reused)
    q2, c2, d2 = direction_queries(store, cam2, sR12, t12, cam1, cam1, th, rows[1], taken2, variant, reused)
    b1, e1 = LM.window_best_ungated(oracle, sides[1]["kps"], sides[1]["desc"], sides[1]["gp"], q1, d1)
    b2, e2 = LM.window_best_ungated(oracle, sides[0]["kps"], sides[0]["desc"], sides[0]["gp"], q2, d2)
    if variant == "levels_plus":
        q1["max_level"] -= (q1["flags"] & Q_ACTIVE)
        q2["max_level"] -= (q2["flags"] & Q_ACTIVE)
    match, nfound = agree(b1, e1, b2, e2, th_high, variant)
    return dict(q=(q1, q2), code=(c1, c2), qdesc=(d1, d2), best=(b1, b2), dist=(e1, e2),
                n_active=np.array([(c1 == ACTIVE).sum(), (c2 == ACTIVE).sum()], np.int32), match12=match, nfound=nfound,
                sim=(sR21, t21, sR12, t12))
