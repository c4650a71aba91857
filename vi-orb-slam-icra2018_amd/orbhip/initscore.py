"""Python mirror of the initialiser's hypothesis scoring (include/orbhip.h, orbhip_init_score[_device]):
the 2 x mMaxIterations CheckHomography / CheckFundamental calls of one Initializer::Initialize attempt as one device call.  All
arithmetic runs in liborbhip."""
import numpy as np

from . import capi
from .capi import KP_DTYPE, _p, check

f32 = np.float32
BEST_DTYPE = np.dtype([("score", "<f4"), ("it", "<i4"), ("ninliers", "<i4")])   # orbhip_init_best


def _hyp(m):
    """[n][9] float32 from anything shaped (n, 3, 3) / (n, 9); None or empty: no hypotheses."""
    if m is None:
        return np.zeros((0, 9), f32)
    return np.ascontiguousarray(m, f32).reshape(-1, 9)


def init_score(ctx, kps1_un, kps2_un, match12, H21, H12, F21, sigma=1.0, out=None, want_scores=True):
    """orbhip_init_score: (scores [nH + nF] or None, best [2] of BEST_DTYPE, inliers [2][n1] uint8).  out: (scores, best, inliers)
    arrays the library writes in place (scores may be None); they may be longer than the call needs."""
    k1, k2 = np.ascontiguousarray(kps1_un, KP_DTYPE), np.ascontiguousarray(kps2_un, KP_DTYPE)
    m = np.ascontiguousarray(match12, np.int32)
    assert len(m) == len(k1)
    h21, h12, f21 = _hyp(H21), _hyp(H12), _hyp(F21)
    assert len(h21) == len(h12)
    n1, nh, nf = len(k1), len(h21), len(f21)
    if out is None:
        scores = np.zeros(nh + nf, f32) if want_scores else None
        best, inl = np.zeros(2, BEST_DTYPE), np.zeros((2, n1), np.uint8)
    else:
        scores, best, inl = out
        assert best.dtype == BEST_DTYPE and inl.dtype == np.uint8 and (scores is None or scores.dtype == f32)
    check(capi.load().orbhip_init_score(ctx.handle, _p(k1) if n1 else None, n1, _p(k2) if len(k2) else None, len(k2),
                                        _p(m) if n1 else None, _p(h21) if nh else None, _p(h12) if nh else None, nh,
                                        _p(f21) if nf else None, nf, f32(sigma), _p(scores), _p(best), _p(inl)), ctx.handle,
          "orbhip_init_score")
    return scores, best, inl


def init_score_device(ctx, d_kps1_un, d_cnt1, cap1, d_kps2_un, d_cnt2, cap2, B, d_match12, d_H21, d_H12, nH, d_F21, nF, sigma,
                      d_scores, d_best, d_inliers):
    """Raw device pointers (ints / c_void_p); asynchronous."""
    check(capi.load().orbhip_init_score_device(ctx.handle, d_kps1_un, d_cnt1, cap1, d_kps2_un, d_cnt2, cap2, B, d_match12, d_H21, d_H12,
                                               nH, d_F21, nF, f32(sigma), d_scores, d_best, d_inliers), ctx.handle,
          "orbhip_init_score_device")
