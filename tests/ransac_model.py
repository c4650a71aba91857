"""Independent model of orbhip_pnp_score / orbhip_sim3_score: PnPsolver::CheckInliers (ref: src/PnPsolver.cc:308-339),
Sim3Solver::CheckInliers + Project (src/Sim3Solver.cc:340-403) and the bookkeeping around them (:209-225, :183-200), restated in
numpy from the arithmetic.  Every line below is one numpy ufunc on float64 or float32 arrays, i.e. one IEEE operation per element,
rounded on its own, in the source's left-to-right order; the selection rules are the reference's loops.

The `variant` arguments exist for the guard tests only: they evaluate the same formulas with one plausible other rounding, to show
that the guard scene tells the two apart."""
import numpy as np

f32, f64 = np.float32, np.float64


def _f32(a):
    return np.asarray(a, f32)


def pnp_error2(Rt, P3Dw, P2D, cam, variant=None):
    """error2 [N] float32 of one hypothesis Rt[12] (R row-major | t, float64).  variant "float_div": invZc as one float division."""
    h = np.asarray(Rt, f64).ravel()
    X3 = _f32(P3Dw).reshape(-1, 3)
    uv = _f32(P2D).reshape(-1, 2)
    X, Y, Z = X3[:, 0].astype(f64), X3[:, 1].astype(f64), X3[:, 2].astype(f64)
    fu, fv, uc, vc = (f64(v) for v in cam)
    with np.errstate(all="ignore"):
        def row(r):
            a = h[3 * r] * X
            b = h[3 * r + 1] * Y
            s = a + b
            c = h[3 * r + 2] * Z
            s = s + c
            return s + h[9 + r]
        Xc = row(0).astype(f32)
        Yc = row(1).astype(f32)
        zc = row(2)
        if variant == "float_div":
            invZc = f32(1.0) / zc.astype(f32)
        else:
            invZc = (f64(1.0) / zc).astype(f32)
        ue = fu * Xc.astype(f64)
        ue = ue * invZc.astype(f64)
        ue = uc + ue
        ve = fv * Yc.astype(f64)
        ve = ve * invZc.astype(f64)
        ve = vc + ve
        dx = (uv[:, 0].astype(f64) - ue).astype(f32)
        dy = (uv[:, 1].astype(f64) - ve).astype(f32)
        xx = dx * dx
        yy = dy * dy
        return xx + yy


def pnp_flags(Rt, P3Dw, P2D, max_err, cam, variant=None):
    with np.errstate(all="ignore"):
        return (pnp_error2(Rt, P3Dw, P2D, cam, variant) < _f32(max_err)).astype(np.uint8)


def _project(T, X, K, variant):
    """Project(X, T, K) for T[12] (3x4 row-major) -> (u, v) float32 [N].  variant "float_gemm": the gemm accumulated in float."""
    T = _f32(T).ravel()
    X = _f32(X).reshape(-1, 3)
    fx, fy, cx, cy = (f32(v) for v in K)
    acc = f32 if variant == "float_gemm" else f64
    Pc = []
    with np.errstate(all="ignore"):
        for r in range(3):
            s = np.zeros(len(X), acc)
            for k in range(3):
                p = acc(T[4 * r + k]) * X[:, k].astype(acc)
                s = s + p
            Pc.append((s + acc(T[4 * r + 3])).astype(f32))
        invz = f32(1.0) / Pc[2]
        x = Pc[0] * invz
        y = Pc[1] * invz
        u = fx * x
        u = u + cx
        v = fy * y
        v = v + cy
    return u, v


def _dot2(d0, d1, variant):
    acc = f32 if variant == "float_dot" else f64
    with np.errstate(all="ignore"):
        a = d0.astype(acc) * d0.astype(acc)
        b = d1.astype(acc) * d1.astype(acc)
        return (a + b).astype(f32)


def sim3_errors(T, X3Dc1, X3Dc2, P1im1, P2im2, K1, K2, variant=None):
    """(err1, err2) [N] float32 of one hypothesis T[24] (the 3x4 block of T12 | of T21)."""
    T = _f32(T).ravel()
    p1, p2 = _f32(P1im1).reshape(-1, 2), _f32(P2im2).reshape(-1, 2)
    with np.errstate(all="ignore"):
        u, v = _project(T[:12], X3Dc2, K1, variant)                 # vP2im1
        err1 = _dot2(p1[:, 0] - u, p1[:, 1] - v, variant)
        u, v = _project(T[12:], X3Dc1, K2, variant)                 # vP1im2
        err2 = _dot2(u - p2[:, 0], v - p2[:, 1], variant)
    return err1, err2


def sim3_flags(T, X3Dc1, X3Dc2, P1im1, P2im2, max_err1, max_err2, K1, K2, variant=None):
    e1, e2 = sim3_errors(T, X3Dc1, X3Dc2, P1im1, P2im2, K1, K2, variant)
    with np.errstate(all="ignore"):
        return ((e1 < _f32(max_err1)) & (e2 < _f32(max_err2))).astype(np.uint8)


def pnp_select(counts, min_inliers, best_in=0, R=None):
    """The loop of PnPsolver::iterate (:209-225) over the counts: (n_records, best_out, record indices, record counts), the lists cut
    to R entries."""
    best, rec = int(best_in), []
    for h, c in enumerate(counts):
        c = int(c)
        if c >= min_inliers:
            if c > best:
                best = c
                rec.append((h, c))
    kept = rec if R is None else rec[:R]
    return len(rec), best, [h for h, _ in kept], [c for _, c in kept]


def sim3_select(counts, min_inliers, best_in=0):
    """The loop of Sim3Solver::iterate (:183-200): (winner, ninliers, best_it, best_out)."""
    best, best_it = int(best_in), -1
    for h, c in enumerate(counts):
        c = int(c)
        if c >= best:
            best, best_it = c, h
            if c > min_inliers:
                return h, c, h, best
    return -1, 0, best_it, best


def pnp_evaluate(P3Dw, P2D, max_err, cam, Rt, min_inliers, best_in=0, R=8):
    """Everything orbhip_pnp_score returns: dict(counts [M], n_records, best_out, rec_idx, rec_cnt, rec_flags [len(rec_idx)][N],
    flags [M][N])."""
    Rt = np.asarray(Rt, f64).reshape(-1, 12)
    N = len(_f32(max_err).ravel())
    flags = np.stack([pnp_flags(h, P3Dw, P2D, max_err, cam) for h in Rt]) if len(Rt) else np.zeros((0, N), np.uint8)
    counts = flags.sum(1).astype(np.int32)
    n, best, idx, cnt = pnp_select(counts, min_inliers, best_in, R)
    return dict(counts=counts, n_records=n, best_out=best, rec_idx=idx, rec_cnt=cnt, rec_flags=flags[idx].reshape(len(idx), N), flags=flags)


def sim3_evaluate(X3Dc1, X3Dc2, P1im1, P2im2, max_err1, max_err2, K1, K2, T, min_inliers, best_in=0):
    """Everything orbhip_sim3_score returns: dict(counts [M], winner, ninliers, best_it, best_out, win_flags [N], flags [M][N])."""
    T = _f32(T).reshape(-1, 24)
    N = len(_f32(max_err1).ravel())
    flags = (np.stack([sim3_flags(h, X3Dc1, X3Dc2, P1im1, P2im2, max_err1, max_err2, K1, K2) for h in T]) if len(T)
             else np.zeros((0, N), np.uint8))
    counts = flags.sum(1).astype(np.int32)
    w, n, it, best = sim3_select(counts, min_inliers, best_in)
    return dict(counts=counts, winner=w, ninliers=n, best_it=it, best_out=best, win_flags=flags[w] if w >= 0 else np.zeros(N, np.uint8),
                flags=flags)
