"""Seeded scenes for the initialiser-scoring tests: two frames' undistorted keypoints, a vnMatches12 with unmatched entries at the
front, in the middle and at the end, and hypotheses made by perturbing the true model.  Pure numpy, no device."""
import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
W, H = 640, 480
K = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]])
H_TRUE = np.array([[1.02, 0.015, 6.0], [-0.01, 0.99, -4.0], [2.0e-5, -1.0e-5, 1.0]])
F_DEGENERATE = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)      # pure sideways translation: the error is the vertical offset


def keypoints(xy):
    k = np.zeros(len(xy), KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, f32)[:, 0], np.asarray(xy, f32)[:, 1]
    k["size"], k["angle"] = 31.0, -1.0
    return k


def _frames(p1, p2, extra1, extra2, rng):
    """Frame 1: the N matched points in order with extra1 unmatched features spread over the front, the middle and the end;
    frame 2: the matched points and extra2 others in a random order.  -> kps1, kps2, match12."""
    N = len(p1)
    front, mid = extra1 // 3, extra1 // 3
    end = extra1 - front - mid
    cut = N // 2
    others1 = rng.uniform([0, 0], [W, H], (extra1, 2))
    xy1 = np.concatenate([others1[:front], p1[:cut], others1[front:front + mid], p1[cut:], others1[front + mid:]])
    slot1 = np.concatenate([np.arange(front, front + cut), np.arange(front + mid + cut, front + mid + N)]).astype(np.int64)
    xy2 = np.concatenate([p2, rng.uniform([0, 0], [W, H], (extra2, 2))])
    perm = rng.permutation(len(xy2))                  # frame-2 feature perm[k] is xy2 row k
    where = np.empty(len(xy2), np.int64)
    where[perm] = np.arange(len(xy2))
    xy2 = xy2[where] if len(xy2) else xy2
    match12 = np.full(len(xy1), -1, np.int32)
    match12[slot1] = perm[:N]
    assert front + mid + end == extra1 and (extra1 < 3 or (match12[0] == -1 and match12[-1] == -1))
    return keypoints(xy1), keypoints(xy2), match12


def planar(N, seed=1, extra1=9, extra2=5, noise=1.0):
    """N matches of a plane seen twice: x2 = H_TRUE x1 plus about `noise` px.  -> kps1, kps2, match12, H_TRUE."""
    rng = np.random.default_rng(seed)
    p1 = rng.uniform([20, 20], [W - 20, H - 20], (N, 2))
    q = np.c_[p1, np.ones(N)] @ H_TRUE.T
    p2 = q[:, :2] / q[:, 2:] + rng.normal(0, noise, (N, 2))
    return _frames(p1, p2, extra1, extra2, rng) + (H_TRUE.copy(),)


def general(N, seed=2, extra1=9, extra2=5, noise=1.0):
    """N matches of a cloud seen from two poses.  -> kps1, kps2, match12, F_true (x2^T F x1 = 0)."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 12, N)]
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([-0.4, 0.05, 0.1])
    x1 = X @ K.T
    x2 = (X @ R.T + t) @ K.T
    p1 = x1[:, :2] / x1[:, 2:] + rng.normal(0, noise / 2, (N, 2))
    p2 = x2[:, :2] / x2[:, 2:] + rng.normal(0, noise / 2, (N, 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return _frames(p1, p2, extra1, extra2, rng) + (F / np.abs(F).max(),)


def perturbed(M, n, seed, rel=2e-4):
    """n hypotheses around the 3x3 M: entry-wise relative perturbations whose size grows with the index from rel / 10 to 20 rel, so
    that good, mediocre and useless hypotheses all occur.  -> [n][9] float32."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 9), f32)
    for i in range(n):
        s = rel * (0.1 + 19.9 * i / max(n - 1, 1))
        out[i] = (M * (1 + rng.normal(0, s, (3, 3)))).astype(f32).ravel()
    return out


def homographies(Htrue, n, seed=11):
    """(H21 [n][9], H12 [n][9]): H12 is the inverse of the float32 H21, formed in double and rounded (any H12 is a valid input)."""
    H21 = perturbed(Htrue, n, seed)
    H12 = np.stack([np.linalg.inv(h.reshape(3, 3).astype(np.float64)).astype(f32).ravel() for h in H21]) if n else np.zeros((0, 9), f32)
    return H21, H12


def fundamentals(Ftrue, n, seed=12):
    return perturbed(Ftrue, n, seed, rel=5e-5)
