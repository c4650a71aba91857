"""Python mirror of the RANSAC inlier checks (include/orbhip.h, orbhip_pnp_score[_device] / orbhip_sim3_score[_device]; DESIGN.md
section 13): PnPsolver::CheckInliers / Sim3Solver::CheckInliers for M hypotheses in one device call, with the solvers' bookkeeping.
All arithmetic runs in liborbhip."""
import ctypes as C

import numpy as np

from . import capi
from .capi import _p, check

f32, f64, i32 = np.float32, np.float64, np.int32
PNP_RESULT = np.dtype([("n_records", "<i4"), ("best_out", "<i4")])                                       # orbhip_pnp_result
SIM3_RESULT = np.dtype([("winner", "<i4"), ("ninliers", "<i4"), ("best_it", "<i4"), ("best_out", "<i4")])   # orbhip_sim3_result


def _a(x, dtype, width):
    return np.ascontiguousarray(x, dtype).reshape(-1, width)


def pnp_hypotheses(R, t):
    """[M][12] float64 from rotations shaped (M, 3, 3) / (M, 9) and translations (M, 3): R row-major, then t."""
    R, t = _a(R, f64, 9), _a(t, f64, 3)
    assert len(R) == len(t)
    return np.ascontiguousarray(np.concatenate([R, t], 1))


def sim3_hypotheses(T12, T21):
    """[M][24] float32 from T12 / T21 shaped (M, 4, 4), (M, 3, 4) or (M, 12): the two 3x4 blocks, row-major."""
    def block(T):
        T = np.asarray(T, f32)
        if T.ndim == 3 and T.shape[1:] == (4, 4):
            T = T[:, :3, :]
        return _a(T, f32, 12)
    a, b = block(T12), block(T21)
    assert len(a) == len(b)
    return np.ascontiguousarray(np.concatenate([a, b], 1))


def pnp_score(ctx, P3Dw, P2D, max_err, cam, Rt, min_inliers, best_in=0, R=8, out=None, want_counts=True):
    """orbhip_pnp_score: (counts [M] or None, res [1] of PNP_RESULT, rec_idx [R], rec_cnt [R], rec_flags [R][N] uint8).  cam: (fu, fv,
    uc, vc); Rt: pnp_hypotheses().  out: the five arrays the library writes in place (counts may be None); they may be longer than
    the call needs.  Entries from min(n_records, R) on keep what they held (-1 / 0 in fresh arrays)."""
    X, uv, me = _a(P3Dw, f32, 3), _a(P2D, f32, 2), np.ascontiguousarray(max_err, f32).ravel()
    Rt = _a(Rt, f64, 12)
    N, M = len(X), len(Rt)
    assert len(uv) == N and len(me) == N
    if out is None:
        rows = max(int(R), 1)
        out = (np.zeros(M, i32) if want_counts else None, np.zeros(1, PNP_RESULT), np.full(rows, -1, i32), np.zeros(rows, i32),
               np.zeros((rows, N), np.uint8))
    counts, res, idx, cnt, flags = out
    assert res.dtype == PNP_RESULT and idx.dtype == i32 and cnt.dtype == i32 and flags.dtype == np.uint8
    assert counts is None or counts.dtype == i32
    check(capi.load().orbhip_pnp_score(ctx.handle, _p(X) if N else None, _p(uv) if N else None, _p(me) if N else None, N, *map(float, cam),
                                       _p(Rt) if M else None, M, int(min_inliers), int(best_in), int(R), _p(counts), _p(res), _p(idx),
                                       _p(cnt), _p(flags)), ctx.handle, "orbhip_pnp_score")
    return out


def sim3_score(ctx, X3Dc1, X3Dc2, P1im1, P2im2, max_err1, max_err2, K1, K2, T, min_inliers, best_in=0, out=None, want_counts=True):
    """orbhip_sim3_score: (counts [M] or None, res [1] of SIM3_RESULT, flags [N] uint8).  K1 / K2: (fx, fy, cx, cy); T:
    sim3_hypotheses().  out: the three arrays the library writes in place."""
    X1, X2, p1, p2 = _a(X3Dc1, f32, 3), _a(X3Dc2, f32, 3), _a(P1im1, f32, 2), _a(P2im2, f32, 2)
    m1, m2 = np.ascontiguousarray(max_err1, f32).ravel(), np.ascontiguousarray(max_err2, f32).ravel()
    T = _a(T, f32, 24)
    k1, k2 = np.ascontiguousarray(K1, f32).ravel(), np.ascontiguousarray(K2, f32).ravel()
    N, M = len(X1), len(T)
    assert len(X2) == N and len(p1) == N and len(p2) == N and len(m1) == N and len(m2) == N and len(k1) == 4 and len(k2) == 4
    if out is None:
        out = (np.zeros(M, i32) if want_counts else None, np.zeros(1, SIM3_RESULT), np.zeros(N, np.uint8))
    counts, res, flags = out
    assert res.dtype == SIM3_RESULT and flags.dtype == np.uint8 and (counts is None or counts.dtype == i32)
    q = lambda a: _p(a) if N else None
    check(capi.load().orbhip_sim3_score(ctx.handle, q(X1), q(X2), q(p1), q(p2), q(m1), q(m2), N, _p(k1), _p(k2), _p(T) if M else None, M,
                                        int(min_inliers), int(best_in), _p(counts), _p(res), _p(flags)), ctx.handle, "orbhip_sim3_score")
    return out


def _host_i32(a, B):
    a = np.ascontiguousarray(a, i32).ravel()
    assert len(a) == B
    return a


def pnp_score_device(ctx, d_P3Dw, d_P2D, d_max_err, off, cam, d_Rt, M, min_inliers, best_in, R, d_counts, d_res, d_rec_idx, d_rec_cnt,
                     d_rec_flags):
    """Raw device pointers (ints / c_void_p) for the d_ arguments; off [B + 1], min_inliers [B], best_in [B] or None: host arrays.
    Asynchronous."""
    off = np.ascontiguousarray(off, i32).ravel()
    B = len(off) - 1
    mi = _host_i32(min_inliers, B)
    bi = None if best_in is None else _host_i32(best_in, B)
    check(capi.load().orbhip_pnp_score_device(ctx.handle, d_P3Dw, d_P2D, d_max_err, _p(off), B, *map(float, cam), d_Rt, int(M), _p(mi),
                                              _p(bi), int(R), d_counts, d_res, d_rec_idx, d_rec_cnt, d_rec_flags), ctx.handle,
          "orbhip_pnp_score_device")


def sim3_score_device(ctx, d_X3Dc1, d_X3Dc2, d_P1im1, d_P2im2, d_max_err1, d_max_err2, off, K1, K2, d_T, M, min_inliers, best_in,
                      d_counts, d_res, d_flags):
    off = np.ascontiguousarray(off, i32).ravel()
    B = len(off) - 1
    mi = _host_i32(min_inliers, B)
    bi = None if best_in is None else _host_i32(best_in, B)
    k1, k2 = np.ascontiguousarray(K1, f32).ravel(), np.ascontiguousarray(K2, f32).ravel()
    check(capi.load().orbhip_sim3_score_device(ctx.handle, d_X3Dc1, d_X3Dc2, d_P1im1, d_P2im2, d_max_err1, d_max_err2, _p(off), B, _p(k1),
                                               _p(k2), d_T, int(M), _p(mi), _p(bi), d_counts, d_res, d_flags), ctx.handle,
          "orbhip_sim3_score_device")
