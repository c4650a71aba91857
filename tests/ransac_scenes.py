"""Seeded scenes for the RANSAC-scoring tests: a camera pose with N 3D-2D correspondences (PnP) and a similarity between two key
frames with N 3D-3D correspondences (Sim3), a share of outliers, and M hypotheses made by perturbing the true model with a size that
grows with the index -- so the counts spread from about N down to 0 -- with every seventh hypothesis a copy of an earlier one, so
that equal counts occur.  Pure numpy, no device."""
import numpy as np

import ransac_model as M

f32, f64 = np.float32, np.float64
CAM = (458.654, 457.296, 367.215, 248.375)            # fu, fv, uc, vc
K1 = (458.654, 457.296, 367.215, 248.375)             # fx, fy, cx, cy of key frame 1
K2 = (435.2, 435.2, 320.0, 240.0)
TH2 = f32(5.991)


def _rot(w):
    """Rodrigues: rotation matrix of the angle-axis vector w (float64)."""
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _sigma2(rng, N):
    """mvLevelSigma2 of random octaves: 1.2^(2 level) as the extractor's float table holds it."""
    table = np.ones(8, f32)
    for i in range(1, 8):
        table[i] = f32(f32(f32(1.2) ** i) * f32(f32(1.2) ** i))
    return table[rng.integers(0, 8, N)]


def _ties(h):
    for i in range(7, len(h), 7):
        h[i] = h[i - 3]
    return h


def pnp(N, Mhyp, seed=1, outliers=0.3):
    """-> dict(P3Dw [N][3], P2D [N][2], max_err [N], cam, Rt [M][12] float64, Rt_true [12])."""
    rng = np.random.default_rng(seed)
    R0, t0 = _rot(np.array([0.05, -0.08, 0.02])), np.array([0.2, -0.1, 0.4])
    Xc = np.c_[rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 12, N)]
    Xw = ((Xc - t0) @ R0).astype(f32)                                     # R0^T (Xc - t0)
    fu, fv, uc, vc = CAM
    uv = np.c_[fu * Xc[:, 0] / Xc[:, 2] + uc, fv * Xc[:, 1] / Xc[:, 2] + vc] + rng.normal(0, 0.7, (N, 2))
    bad = rng.random(N) < outliers
    uv[bad] = rng.uniform([0, 0], [752, 480], (int(bad.sum()), 2))
    max_err = (_sigma2(rng, N) * TH2).astype(f32)                         # mvSigma2[i] * th2, a float product
    Rt = np.empty((Mhyp, 12), f64)
    for i in range(Mhyp):
        s = 0.0 if Mhyp == 1 else (i / (Mhyp - 1)) ** 2
        R = _rot(rng.normal(0, 0.03 * s + 1e-5, 3)) @ R0
        Rt[i] = np.r_[R.ravel(), t0 + rng.normal(0, 0.3 * s + 1e-5, 3)]
    return dict(P3Dw=Xw, P2D=uv.astype(f32), max_err=max_err, cam=CAM, Rt=_ties(Rt), Rt_true=np.r_[R0.ravel(), t0])


def _T(s, R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, t
    return T


def _to_image(X, K):
    """Sim3Solver::FromCameraToImage in float32 (the result is input data: any rounding of it is a valid input)."""
    X = np.asarray(X, f32)
    fx, fy, cx, cy = (f32(v) for v in K)
    invz = f32(1.0) / X[:, 2]
    return np.stack([fx * (X[:, 0] * invz) + cx, fy * (X[:, 1] * invz) + cy], 1).astype(f32)


def sim3(N, Mhyp, seed=2, outliers=0.3):
    """-> dict(X3Dc1, X3Dc2 [N][3], P1im1, P2im2 [N][2], max_err1, max_err2 [N], K1, K2, T [M][24] float32)."""
    rng = np.random.default_rng(seed)
    s0, R0, t0 = 1.07, _rot(np.array([0.04, 0.1, -0.03])), np.array([0.3, 0.05, -0.2])
    X1 = np.c_[rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 12, N)]
    X2 = ((X1 - t0) @ R0) / s0 + rng.normal(0, 0.01, (N, 3))              # X1 = s0 R0 X2 + t0
    bad = rng.random(N) < outliers
    X2[bad] = np.c_[rng.uniform(-3, 3, int(bad.sum())), rng.uniform(-2, 2, int(bad.sum())), rng.uniform(4, 12, int(bad.sum()))]
    X1, X2 = X1.astype(f32), X2.astype(f32)
    e1 = (9.210 * _sigma2(rng, N).astype(f64)).astype(f32)
    e2 = (9.210 * _sigma2(rng, N).astype(f64)).astype(f32)
    T = np.empty((Mhyp, 24), f32)
    for i in range(Mhyp):
        a = 0.0 if Mhyp == 1 else (i / (Mhyp - 1)) ** 2
        T12 = _T(s0 * (1 + rng.normal(0, 0.02 * a + 1e-6)), _rot(rng.normal(0, 0.03 * a + 1e-5, 3)) @ R0, t0 + rng.normal(0, 0.3 * a + 1e-5, 3))
        T21 = np.linalg.inv(T12)
        T[i] = np.r_[T12[:3].ravel(), T21[:3].ravel()].astype(f32)
    return dict(X3Dc1=X1, X3Dc2=X2, P1im1=_to_image(X1, K1), P2im2=_to_image(X2, K2), max_err1=e1, max_err2=e2, K1=K1, K2=K2, T=_ties(T))


def _one_ulp(x, up):
    x = np.asarray(x, f32)
    return np.where(up, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))).astype(f32)


GUARD_SEED = 5        # tests/test_ransac_model.py asserts that this seed separates the roundings


def pnp_guard(N=257, Mhyp=9, seed=GUARD_SEED):
    """The PnP scene with max_err[i] = the model's own error2 of point i under hypothesis 0, one ulp up (even i: an inlier) or down
    (odd i: not one): any other rounding of error2 that moves it by an ulp flips a flag of hypothesis 0."""
    s = pnp(N, Mhyp, seed)
    e = M.pnp_error2(s["Rt"][0], s["P3Dw"], s["P2D"], s["cam"])
    s["max_err"] = _one_ulp(e, np.arange(N) % 2 == 0)
    return s


def sim3_guard(N=257, Mhyp=9, seed=GUARD_SEED):
    s = sim3(N, Mhyp, seed)
    e1, e2 = M.sim3_errors(s["T"][0], s["X3Dc1"], s["X3Dc2"], s["P1im1"], s["P2im2"], s["K1"], s["K2"])
    up = np.arange(N) % 2 == 0
    s["max_err1"], s["max_err2"] = _one_ulp(e1, up), _one_ulp(e2, up)
    return s


def pnp_args(s):
    return s["P3Dw"], s["P2D"], s["max_err"], s["cam"], s["Rt"]


def sim3_args(s):
    return s["X3Dc1"], s["X3Dc2"], s["P1im1"], s["P2im2"], s["max_err1"], s["max_err2"], s["K1"], s["K2"], s["T"]


def scene_bytes(kind, s, min_inliers, best_in):
    """The scene file of tests/native_ransac: int32 kind (0 PnP, 1 Sim3), N, M, min_inliers, best_in, then the arrays in argument
    order (PnP: P3Dw, P2D, max_err float32, cam float64[4], Rt float64; Sim3: the six point arrays, K1, K2, T float32)."""
    if kind == "pnp":
        head = np.array([0, len(s["max_err"]), len(s["Rt"]), min_inliers, best_in], np.int32)
        parts = [s["P3Dw"].astype(f32), s["P2D"].astype(f32), s["max_err"].astype(f32), np.asarray(s["cam"], f64), np.asarray(s["Rt"], f64)]
    else:
        head = np.array([1, len(s["max_err1"]), len(s["T"]), min_inliers, best_in], np.int32)
        parts = [np.asarray(s[k], f32) for k in ("X3Dc1", "X3Dc2", "P1im1", "P2im2", "max_err1", "max_err2", "K1", "K2", "T")]
    return head.tobytes() + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
