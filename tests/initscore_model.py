"""Independent model of orbhip_init_score: Initializer::CheckHomography / CheckFundamental (ref: src/Initializer.cc:305-468) and
the `currentScore > score` updates of FindHomography / FindFundamental (:148-171, :199-222), restated in numpy float32 from the
arithmetic.  Every numpy operation below is one IEEE float32 operation per element (no fused multiply-add, no double
intermediate), written in the source's left-to-right order.  The score is formed by an explicit sequential loop over the terms
in match order -- never by np.sum, whose pairwise order is a different float sum."""
import numpy as np

f32 = np.float32
TH_H = f32(5.991)          # :333
TH_F = f32(3.841)          # :408
TH_SCORE = f32(5.991)      # :409
BEST_DTYPE = np.dtype([("score", "<f4"), ("it", "<i4"), ("ninliers", "<i4")])


def inv_sigma_square(sigma):
    """`const float invSigmaSquare = 1.0/(sigma*sigma)`: the product in float, the quotient in double, rounded to float."""
    s = f32(sigma)
    with np.errstate(all="ignore"):
        return f32(1.0 / float(f32(s * s)))


def pairs(kps1, kps2, match12, n2=None):
    """mvMatches12 (:54-63): (frame-1 indices ascending, u1, v1, u2, v2).  n2: entries outside [0, n2) count as unmatched too
    (the device form's rule); by default only negative ones do."""
    m = np.asarray(match12, np.int64)
    ok = m >= 0
    if n2 is not None:
        ok &= m < n2
    idx = np.nonzero(ok)[0]
    j = m[idx]
    return idx, kps1["x"][idx].astype(f32), kps1["y"][idx].astype(f32), kps2["x"][j].astype(f32), kps2["y"][j].astype(f32)


def _transfer_chi(M, us, vs, ud, vd, inv):
    """chiSquare of (us, vs) carried through the 3x3 M against (ud, vd) (:352-358 / :368-374)."""
    m = [f32(v) for v in np.asarray(M, f32).ravel()]
    one = f32(1.0)
    winv = one / ((m[6] * us + m[7] * vs) + m[8])            # 1.0 / (float): one correctly rounded float division
    x = ((m[0] * us + m[1] * vs) + m[2]) * winv
    y = ((m[3] * us + m[4] * vs) + m[5]) * winv
    dx, dy = ud - x, vd - y
    return (dx * dx + dy * dy) * inv


def chi_h(H21, H12, u1, v1, u2, v2, inv):
    """(chiSquare1, chiSquare2) per match: image 1 through H12 first, image 2 through H21 second."""
    with np.errstate(all="ignore"):
        return _transfer_chi(H12, u2, v2, u1, v1, inv), _transfer_chi(H21, u1, v1, u2, v2, inv)


def chi_f(F21, u1, v1, u2, v2, inv):
    """(chiSquare1, chiSquare2) per match: the line of x1 in image 2 first (:428-436), the line of x2 in image 1 second (:446-454)."""
    f = [f32(v) for v in np.asarray(F21, f32).ravel()]
    f11, f12, f13, f21, f22, f23, f31, f32_, f33 = f
    with np.errstate(all="ignore"):
        a2 = (f11 * u1 + f12 * v1) + f13
        b2 = (f21 * u1 + f22 * v1) + f23
        c2 = (f31 * u1 + f32_ * v1) + f33
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv
        a1 = (f11 * u2 + f21 * v2) + f31
        b1 = (f12 * u2 + f22 * v2) + f32_
        c1 = (f13 * u2 + f23 * v2) + f33
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv
    return chi1, chi2


def terms(chi1, chi2, th):
    """The 2N candidate terms of one hypothesis in the order the reference adds them, and which of them it skips:
    (values [2N], skipped [2N], inlier [N]).  `chiSquare > th` as written: a NaN is not skipped."""
    with np.errstate(all="ignore"):
        chi = np.stack([chi1, chi2], 1).astype(f32).ravel()
        skipped = chi > th
        values = (TH_SCORE - chi).astype(f32)
    return values, skipped, ~skipped.reshape(-1, 2).any(1)


def sequential_sum(values, skipped):
    """`score += th - chiSquare` down the rows of values [nhyp][K] at once: one float32 addition per term and hypothesis, in
    term order, from 0.0f; a skipped term leaves the score as it is."""
    values, skipped = np.atleast_2d(values), np.atleast_2d(skipped)
    s = np.zeros(values.shape[0], f32)
    with np.errstate(all="ignore"):
        for k in range(values.shape[1]):
            s = np.where(skipped[:, k], s, (s + values[:, k]).astype(f32))
    return s


def winner(scores):
    """`if(currentScore>score)` from score = 0 over the iterations in order: (score, it); it = -1 when nothing beat 0."""
    best, it = f32(0.0), -1
    for i, s in enumerate(np.asarray(scores, f32)):
        if s > best:
            best, it = s, i
    return best, it


def evaluate(kps1, kps2, match12, H21, H12, F21, sigma, n2=None):
    """Everything orbhip_init_score returns: dict(scores [nH + nF], best [2] records, inliers [2][n1] bytes, chi=[per model: list of
    (chi1, chi2) per hypothesis])."""
    idx, u1, v1, u2, v2 = pairs(kps1, kps2, match12, n2)
    inv = inv_sigma_square(sigma)
    H21 = np.zeros((0, 9), f32) if H21 is None else np.asarray(H21, f32).reshape(-1, 9)
    H12 = np.zeros((0, 9), f32) if H12 is None else np.asarray(H12, f32).reshape(-1, 9)
    F21 = np.zeros((0, 9), f32) if F21 is None else np.asarray(F21, f32).reshape(-1, 9)
    n1 = len(match12)
    out_scores, best, inliers, chis = [], np.zeros(2, BEST_DTYPE), np.zeros((2, n1), np.uint8), []
    for model, (hyps, th) in enumerate(((list(zip(H21, H12)), TH_H), ([(F,) for F in F21], TH_F))):
        per = []
        for h in hyps:
            c1, c2 = chi_h(h[0], h[1], u1, v1, u2, v2, inv) if model == 0 else chi_f(h[0], u1, v1, u2, v2, inv)
            per.append((c1, c2) + terms(c1, c2, th))
        chis.append([(p[0], p[1]) for p in per])
        if per:
            sc = sequential_sum(np.stack([p[2] for p in per]), np.stack([p[3] for p in per]))
        else:
            sc = np.zeros(0, f32)
        out_scores.append(sc)
        s, it = winner(sc)
        best[model] = (s, it, 0)
        if it >= 0:
            inl = per[it][4]
            inliers[model, idx] = inl
            best[model]["ninliers"] = int(inl.sum())
    return dict(scores=np.concatenate(out_scores).astype(f32), best=best, inliers=inliers, chi=chis, idx=idx)
