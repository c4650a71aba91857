"""Independent model of LoopClosing's two projection searches up to the point where the map is edited, written from the cited lines:
ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, vpPoints, vpMatched, th) (ref: src/ORBmatcher.cc:290-403) and
ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (ref: :977-1080), with the union of
LoopClosing::ComputeSim3 (ref: src/LoopClosing.cc:404-424) in front of the first.

The projection of both (:320-360, :1008-1049) is that of Fuse(pKF, vpMapPoints, th) line for line (:850-888), so it is taken from
tests/fuse_model.py (numpy, one rounding per stated operation); there is no right coordinate, proj_xr is 0.  What differs is written
out here: the decomposition of the similarity (:299-303, :986-990), "already in the key frame" as a set of points (:306-307, :993),
the window search WITHOUT a chi-square gate (:1062-1079) and the sequential claim (:372-398: a feature that holds a match is closed
to the points after it, the best distance must not exceed TH_LOW)."""
import numpy as np

import fuse_model as FM
from fuse_model import ACTIVE, BAD, EXITS, MP_BAD, NO_POINT, Q_ACTIVE, SKIPPED, TH_LOW, UNKNOWN, Store, tally   # noqa: F401

f32, f64 = np.float32, np.float64


def sim3(s, R, t):
    """Scw = [s R | s t] as the float matrix LoopClosing holds."""
    S = np.eye(4, dtype=f32)
    S[:3, :3] = (f64(s) * np.asarray(R, f64)).astype(f32)
    S[:3, 3] = (f64(s) * np.asarray(t, f64)).astype(f32)
    return S


def decompose_sim3(Scw):
    """(Rcw, tcw, Ow, scw) of :986-990: scw = sqrt(row 0 . row 0) (a double dot product, the root rounded to float), Rcw = sRcw / scw
    and tcw = t / scw (OpenCV multiplies by the double 1 / scw and rounds once), Ow = -Rcw' tcw (one gemm: double sums, one rounding)."""
    Scw = np.asarray(Scw, f32)
    dot = f64(0)
    for k in range(3):
        dot = dot + f64(Scw[0, k]) * f64(Scw[0, k])
    scw = f32(np.sqrt(dot))
    inv = f64(1.0) / f64(scw)
    Rcw = (Scw[:3, :3].astype(f64) * inv).astype(f32)
    tcw = (Scw[:3, 3].astype(f64) * inv).astype(f32)
    Ow = np.zeros(3, f32)
    for r in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(Rcw[k, r]) * f64(tcw[k])
        Ow[r] = f32(f64(-1.0) * s)
    return Rcw, tcw, Ow, scw


def held_points(store, row):
    """spAlreadyFound = pKF->GetMapPoints() (:993; src/KeyFrame.cc: the row's points that are not NULL and not bad) as keys; an
    entry whose point the store no longer knows names nothing."""
    if row is None:
        return set()
    return {int(k) for k in row if int(k) and int(k) in store.pts and not (store.pts[int(k)][5] & MP_BAD)}


def queries(store, cam, th, keys, closed_points):
    """The loop head of both searches for the points `keys`: (queries, exit codes, qdesc); proj_xr is 0."""
    skip = np.array([int(k) in closed_points for k in keys], np.uint8)
    q, code, qd = FM.fuse_queries(store, cam, th, keys, skip)
    q["proj_xr"] = 0
    return q, code, qd


def _bits(d):
    return np.unpackbits(np.ascontiguousarray(d, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)


def window_best_ungated(oracle, kps, desc, gp, q, qdesc):
    """:1051-1079 per query: the features of GetFeaturesInArea(u, v, radius) in their order, levels [predicted - 1, predicted], the
    first feature of smallest distance; -1 / 256 when there is none."""
    grid = oracle.grid_build(kps, gp)
    fb, qb = _bits(desc), _bits(qdesc)
    bi, bd = np.full(len(q), -1, np.int32), np.full(len(q), 256, np.int32)
    for i in range(len(q)):
        if not q["flags"][i] & Q_ACTIVE:
            continue
        for idx in oracle.features_in_area(kps, grid, gp, q["u"][i], q["v"][i], q["radius"][i], -1, -1):
            lvl = int(kps["octave"][idx])
            if lvl < q["min_level"][i] or lvl > q["max_level"][i]:
                continue
            d = int(np.abs(fb[idx] - qb[i]).sum())
            if d < bd[i]:
                bd[i], bi[i] = d, idx
    return bi, bd


def claim_search(oracle, kps, desc, gp, q, qdesc, closed, th_high=TH_LOW, trace=None):
    """:362-398 in list order.  closed[idx] != 0: vpMatched[idx] is set.  Returns (nmatches, match[feature] = list index or -1).
    trace (list) receives per active point (i, best feature or -1, best distance, best feature had no feature been closed)."""
    n = len(kps)
    grid = oracle.grid_build(kps, gp)
    fb, qb = _bits(desc), _bits(qdesc)
    taken = np.array(closed, bool).copy() if closed is not None else np.zeros(n, bool)
    match = np.full(n, -1, np.int32)
    nm = 0
    for i in range(len(q)):
        if not q["flags"][i] & Q_ACTIVE:
            continue
        best, bi, free_best, free_bi = 256, -1, 256, -1
        for idx in oracle.features_in_area(kps, grid, gp, q["u"][i], q["v"][i], q["radius"][i], -1, -1):
            lvl = int(kps["octave"][idx])
            if lvl < q["min_level"][i] or lvl > q["max_level"][i]:
                continue
            d = int(np.abs(fb[idx] - qb[i]).sum())
            if d < free_best:
                free_best, free_bi = d, idx
            if taken[idx]:
                continue                            # :375
            if d < best:
                best, bi = d, idx
        if best <= th_high:                         # :394
            match[bi] = i
            taken[bi] = True
            nm += 1
        if trace is not None:
            trace.append((i, bi if best <= th_high else -1, best, free_bi))
    return nm, match


def fuse_sim3(oracle, store, targets, rows, keys):
    """Per target dict(cam, th, kps, desc, gp): (queries, codes, qdesc, n_active, best_idx, best_dist); rows[k] = the target's
    mvpMapPoints as keys, or None."""
    out = []
    for T, row in zip(targets, rows):
        q, code, qd = queries(store, T["cam"], T["th"], keys, held_points(store, row))
        bi, bd = window_best_ungated(oracle, T["kps"], T["desc"], T["gp"], q, qd)
        out.append((q, code, qd, int((code == ACTIVE).sum()), bi, bd))
    return out


def search_loop_points(oracle, store, T, rows, matched_keys, th_high=TH_LOW, trace=None):
    """ComputeSim3's union of `rows` and the claim search over it.  Returns (keys, queries, codes, qdesc, n_active, nmatches, match)."""
    keys = FM.collect(store, rows)
    mk = np.zeros(len(T["kps"]), np.uint64) if matched_keys is None else np.asarray(matched_keys, np.uint64)
    found = {int(k) for k in mk if int(k)}
    q, code, qd = queries(store, T["cam"], T["th"], keys, found)
    na = int((code == ACTIVE).sum())
    if len(T["kps"]) == 0 or len(keys) == 0:
        return keys, q, code, qd, na, 0, np.full(len(T["kps"]), -1, np.int32)
    nm, match = claim_search(oracle, T["kps"], T["desc"], T["gp"], q, qd, mk != 0, th_high, trace)
    return keys, q, code, qd, na, nm, match
