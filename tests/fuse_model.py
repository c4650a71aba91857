"""Independent model of ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) up to the point where the map is
edited (ref: src/ORBmatcher.cc:842-950), written from the cited lines: numpy with one rounding per stated operation (float64 sums,
explicit float32 everywhere else) and the C library's own logf for the level -- not the threshold table the device uses.

The projection (:850-890) differs from the frame searches' (tests/projtrack_model.py) in four places: invz = 1 / z is a float
division; x = xc * invz is rounded before u = fx * x + cx; the image test is KeyFrame::IsInImage, u >= min_x && u < max_x (the
maximum is outside, NaN fails); and the depth sign is tested on z itself.  The window search (:887-950) is restated here too: the
features of KeyFrame::GetFeaturesInArea in their order, levels [predicted - 1, predicted], the chi-square gate on the reprojection
error (7.8 with the right coordinate when mvuRight[idx] >= 0, else 5.99; the float product compared as a double), the first feature
of smallest distance.

Stated divergences: a point with dist3D == 0 or not finite, with a non-finite mfMaxDistance / dist3D, or with
a key the store does not know is inactive."""
import numpy as np

from localmap_model import QUERY_DTYPE, Store, gemm3, predict_scale   # noqa: F401 (Store: re-exported for the tests)

f32, f64 = np.float32, np.float64
Q_ACTIVE, Q_OBSERVED = 1, 2
MP_OBSERVED, MP_BAD = 1, 2
TH_LOW = 50

# why a source entry gives no query, in the order the loop tests (0 = active)
(ACTIVE, NO_POINT, UNKNOWN, BAD, SKIPPED, BEHIND, LEFT, RIGHT, TOP, BOTTOM, NONFINITE, NEAR, FAR, VIEW) = range(14)
EXITS = ("active", "no point", "unknown", "bad", "skipped", "behind", "left", "right", "top", "bottom", "nonfinite", "near", "far", "view")


def project(cam, P, other_association=False):
    """(Pc, invz, u, v) as Fuse computes them (:850-862); other_association: u = (fx * xc) * invz + cx, as the frame searches."""
    P = np.ascontiguousarray(P, f32).reshape(-1, 3)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        Pc = gemm3(cam["Rcw"], P, cam["tcw"])
        invz = f32(1.0) / Pc[:, 2]
        if other_association:
            u = (fx * Pc[:, 0]) * invz + cx
            v = (fy * Pc[:, 1]) * invz + cy
        else:
            x = Pc[:, 0] * invz
            y = Pc[:, 1] * invz
            u = fx * x + cx
            v = fy * y + cy
    assert invz.dtype == f32 and u.dtype == f32 and v.dtype == f32
    return Pc, invz, u, v


def fuse_queries(store, cam, th, keys, skip=None, other_association=False):
    """keys[i] = the i-th source point as a key (0: NULL); skip[i] != 0 = IsInKeyFrame(pKF).  cam: dict as in localmap_model with
    bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY) of the TARGET key frame.  Returns (queries, exit codes, qdesc)."""
    n = len(keys)
    sf = np.asarray(cam["scale_factors"], f32)
    th, mbf = f32(th), f32(cam["mbf"])
    min_x, max_x, min_y, max_y = (f32(b) for b in cam["bounds"])
    q = np.zeros(n, QUERY_DTYPE)
    code = np.zeros(n, np.int32)
    qdesc = np.zeros((n, 32), np.uint8)
    have = []
    for i in range(n):
        k = int(keys[i])
        if k == 0:
            code[i] = NO_POINT
        elif k not in store.pts:
            code[i] = UNKNOWN
        elif store.pts[k][5] & MP_BAD:
            code[i] = BAD                          # :847
        elif skip is not None and skip[i]:
            code[i] = SKIPPED                      # :847 IsInKeyFrame
        else:
            have.append(i)
    if not have:
        return q, code, qdesc
    pts = [store.pts[int(keys[i])] for i in have]
    P = np.stack([p[0] for p in pts])
    Pn = np.stack([p[1] for p in pts])
    Pc, invz, u, v = project(cam, P, other_association)
    with np.errstate(all="ignore"):
        ur = u - mbf * invz                        # :868
        PO = P - np.asarray(cam["Ow"], f32).reshape(1, 3)
        sq, dot = np.zeros(len(P), f64), np.zeros(len(P), f64)
        for k in range(3):
            sq = sq + PO[:, k].astype(f64) * PO[:, k].astype(f64)
            dot = dot + PO[:, k].astype(f64) * Pn[:, k].astype(f64)
        dist = np.sqrt(sq).astype(f32)             # :873 cv::norm
        mn, mx = np.array([p[2] for p in pts], f32), np.array([p[3] for p in pts], f32)
        lo, hi = f32(0.8) * mn, f32(1.2) * mx
        ratio = mx / dist
        half = f64(0.5) * dist.astype(f64)
    assert ur.dtype == f32 and PO.dtype == f32 and lo.dtype == f32 and ratio.dtype == f32 and dot.dtype == f64
    for j, i in enumerate(have):
        if Pc[j, 2] < f32(0.0):
            code[i] = BEHIND                       # :854
        elif u[j] < min_x:
            code[i] = LEFT                         # :865, KeyFrame::IsInImage
        elif u[j] >= max_x:
            code[i] = RIGHT
        elif v[j] < min_y:
            code[i] = TOP
        elif v[j] >= max_y:
            code[i] = BOTTOM
        elif not (u[j] >= min_x and u[j] < max_x and v[j] >= min_y and v[j] < max_y):
            code[i] = NONFINITE                    # NaN fails IsInImage
        elif not (dist[j] > 0 and np.isfinite(dist[j])):
            code[i] = NONFINITE                    # divergence
        elif dist[j] < lo[j]:
            code[i] = NEAR                         # :876
        elif dist[j] > hi[j]:
            code[i] = FAR
        elif dot[j] < half[j]:
            code[i] = VIEW                         # :882
        elif not np.isfinite(ratio[j]):
            code[i] = NONFINITE                    # divergence
        else:
            lv = predict_scale(ratio[j], cam["log_scale_factor"], len(sf))
            q[i] = (u[j], v[j], f32(th * sf[lv]), ur[j], lv - 1, lv, 0.0, Q_ACTIVE | Q_OBSERVED)
            qdesc[i] = pts[j][4]
    return q, code, qdesc


def window_best_gated(oracle, kps, desc, gp, q, qdesc, u_right, sig, stats=None):
    """The loop of :887-950 per query.  stats (dict) counts what each gate decided: mono_pass, mono_out, stereo_pass, stereo_out."""
    grid = oracle.grid_build(kps, gp)
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    qb = np.unpackbits(np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    sig = np.asarray(sig, f32)
    bi = np.full(len(q), -1, np.int32)
    bd = np.full(len(q), 256, np.int32)
    stats = {} if stats is None else stats
    for k in ("mono_pass", "mono_out", "stereo_pass", "stereo_out"):
        stats.setdefault(k, 0)
    for i in range(len(q)):
        if not q["flags"][i] & Q_ACTIVE:
            continue
        for idx in oracle.features_in_area(kps, grid, gp, q["u"][i], q["v"][i], q["radius"][i], -1, -1):
            lvl = int(kps["octave"][idx])
            if lvl < q["min_level"][i] or lvl > q["max_level"][i]:
                continue
            ex, ey = f32(q["u"][i] - kps["x"][idx]), f32(q["v"][i] - kps["y"][idx])
            e2 = f32(f32(ex * ex) + f32(ey * ey))
            if u_right is not None and u_right[idx] >= 0:
                er = f32(q["proj_xr"][i] - u_right[idx])
                out = float(f32(f32(e2 + f32(er * er)) * sig[lvl])) > 7.8
                stats["stereo_out" if out else "stereo_pass"] += 1
            else:
                out = float(f32(e2 * sig[lvl])) > 5.99
                stats["mono_out" if out else "mono_pass"] += 1
            if out:
                continue
            d = int(np.abs(bits[idx] - qb[i]).sum())
            if d < bd[i]:
                bd[i], bi[i] = d, idx
    return bi, bd


def fuse(oracle, store, target, th, keys, skip=None, stats=None):
    """One target: dict(cam, kps, desc, gp, u_right or None, sig).  Returns (queries, codes, qdesc, n_active, best_idx, best_dist)."""
    q, code, qd = fuse_queries(store, target["cam"], th, keys, skip)
    bi, bd = window_best_gated(oracle, target["kps"], target["desc"], target["gp"], q, qd, target["u_right"], target["sig"], stats)
    return q, code, qd, int((code == ACTIVE).sum()), bi, bd


def collect(store, rows):
    """vpFuseCandidates as keys (ref: src/LocalMapping.cc:2563-2580): the rows in order, each in feature order, NULL / unknown / bad
    entries dropped, the first occurrence of a point kept."""
    seen, out = set(), []
    for row in rows:
        for k in row:
            k = int(k)
            if k == 0 or k not in store.pts or store.pts[k][5] & MP_BAD or k in seen:
                continue
            seen.add(k)
            out.append(k)
    return np.array(out, np.uint64)


def tally(code):
    return {EXITS[c]: int((code == c).sum()) for c in range(len(EXITS)) if (code == c).any()}
