"""Independent numpy model of orbhip_map_correct_sim3 and orbhip_map_correct_se3 (include/orbhip.h), written from
the reference's lines as a sequence: LoopClosing::CorrectLoop (ref: src/LoopClosing.cc:523-568) walks the corrected key frames in order,
moves and refreshes each one's points and only then sets its pose; RunGlobalBundleAdjustment (ref: :762-797) carries a point from its
reference key frame's pose before the adjustment to the one after it.  The device call states the first as a rule on ranks instead
(an observer counts as corrected when 0 <= rank < corr); the two formulations check each other.  np.float32 / np.float64 scalars:
every operation is one individually rounded IEEE operation (docs/parity.md, "CorrectLoop").  UpdateNormalAndDepth itself is
refresh_model.normal_depth.  The `variant` arguments compute what a wrong implementation would, for the guard scene that
tests/test_correct_model.py asserts to discriminate.  No device, no liborbhip."""
from fractions import Fraction

import numpy as np

import refresh_model as R

f32, f64 = np.float32, np.float64
MP_OBSERVED, MP_BAD = 1, 2
SIM3D_DTYPE = np.dtype([("q", "<f8", 4), ("t", "<f8", 3), ("s", "<f8")])                       # orbhip_sim3d, q = x y z w
XF_DTYPE = np.dtype([("Siw", SIM3D_DTYPE), ("corrected_Swi", SIM3D_DTYPE)])                    # orbhip_correct_xf
KF_DTYPE = np.dtype([("Ow_before", "<f4", 3), ("Ow_after", "<f4", 3), ("rank", "<i4")])        # orbhip_correct_kf
SE3_DTYPE = np.dtype([("Rcw_before", "<f4", 9), ("tcw_before", "<f4", 3), ("Rwc", "<f4", 9), ("twc", "<f4", 3)])   # orbhip_correct_se3
VARIANTS_SIM3 = ("all_after", "all_before", "own_after", "fused_cross", "float_maps")
bits = R.bits


def _cross_term(a, b, c, d, variant):
    """a*b - c*d: two rounded products and one rounded difference.  "fused_cross": a*b enters the subtraction unrounded (an fma)."""
    if variant == "fused_cross":
        return f64(float(Fraction(float(a)) * Fraction(float(b)) - Fraction(float(c * d))))
    return a * b - c * d


def sim3_map(S, v, variant=None):
    """g2o::Sim3::map (ref: Thirdparty/g2o/g2o/types/sim3.h:144): s*(r*xyz)+t; r*xyz as Eigen 3's Quaternion::_transformVector:
    uv = q.vec x v; uv += uv; (v + w*uv) + q.vec x uv.  v: three scalars of one type.  "float_maps": everything in float."""
    T = f32 if variant == "float_maps" else f64
    qx, qy, qz, qw = (T(x) for x in S["q"])
    t, s = [T(x) for x in S["t"]], T(S["s"])
    x, y, z = (T(c) for c in v)
    with np.errstate(all="ignore"):
        ux, uy, uz = _cross_term(qy, z, qz, y, variant), _cross_term(qz, x, qx, z, variant), _cross_term(qx, y, qy, x, variant)
        ux, uy, uz = ux + ux, uy + uy, uz + uz
        rx = (x + qw * ux) + _cross_term(qy, uz, qz, uy, variant)
        ry = (y + qw * uy) + _cross_term(qz, ux, qx, uz, variant)
        rz = (z + qw * uz) + _cross_term(qx, uy, qy, ux, variant)
        return [s * rx + t[0], s * ry + t[1], s * rz + t[2]]


def correct_point(xf, pos, variant=None):
    """g2oCorrectedSwi.map(g2oSiw.map(toVector3d(P))) rounded to float: pos [3] f32 -> [3] f32."""
    v = sim3_map(xf["Siw"], [f64(c) for c in np.asarray(pos, f32)], variant)   # Converter::toVector3d widens exactly
    v = sim3_map(xf["corrected_Swi"], v, variant)
    return np.array([f32(c) for c in v], f32)                                  # Converter::toCvMat rounds once


def correct_sim3(sc, store=None, variant=None):
    """The whole call over the scene `sc` (make_scene) on `store` (default: the scene's initial values), as the reference's sequence.
    Returns (status, pos, normal, min_dist, max_dist); store is not modified.  variant: one of VARIANTS_SIM3 --
    "all_after": every corrected observer stands at its corrected centre from the start; "all_before": no SetPose ever happens;
    "own_after": a key frame's pose is set before its own points are refreshed."""
    st = store or sc
    P, K, kfs = len(sc["keys"]), len(sc["xf"]), sc["kfs"]
    status = np.zeros(P, np.uint8)
    pos, normal = np.array(st["pos"], f32).copy(), np.array(st["normal"], f32).copy()
    mn, mx = np.array(st["min_dist"], f32).copy(), np.array(st["max_dist"], f32).copy()
    centre = np.array(kfs["Ow_before"], f32).copy()                  # GetCameraCenter() of every key frame before the loop
    if variant == "all_after":
        centre[kfs["rank"] >= 0] = kfs["Ow_after"][kfs["rank"] >= 0]
    for j in range(K):                                               # for(mit=CorrectedSim3.begin(); ...)
        own = kfs["rank"] == j
        if variant == "own_after":
            centre[own] = kfs["Ow_after"][own]
        for p in range(P):                                           # pKFi's points the batch hands to it
            if sc["corr"][p] != j or (st["flags"][p] & MP_BAD):
                continue
            pos[p] = correct_point(sc["xf"][j], pos[p], variant)     # SetWorldPos
            status[p] = 1
            a, b = sc["off"][p], sc["off"][p + 1]
            if b > a:                                                # UpdateNormalAndDepth, with the centres as they are now
                obs = sc["obs_kf"][a:b]
                normal[p], mn[p], mx[p] = R.normal_depth(pos[p], centre[obs], sc["ref_pos"][p], int(sc["ref_level"][p]), sc["sf"],
                                                         sc["nlevels"])
                status[p] = 3
        if variant != "all_before":
            centre[own] = kfs["Ow_after"][own]                       # pKFi->SetPose(correctedTiw)
    return status, pos, normal, mn, mx


def affine(Rm, t, x, variant=None):
    """One gemm R*x + t on CV_32F: products and sums in double from 0.0, t added, rounded once.  "float_accum": all in float."""
    T = f32 if variant == "float_accum" else f64
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            s = T(0)
            for k in range(3):
                s = s + T(Rm[3 * r + k]) * T(x[k])
            out.append(f32(s + T(t[r])))
    return out


def correct_se3(sc, store=None, variant=None):
    """orbhip_map_correct_se3 over the scene (make_se3_scene).  Returns (status, pos)."""
    st = store or sc
    P = len(sc["keys"])
    status, pos = np.zeros(P, np.uint8), np.array(st["pos"], f32).copy()
    for p in range(P):
        if st["flags"][p] & MP_BAD:
            continue
        c = sc["corr"][p]
        if c < 0:
            pos[p] = sc["pos_set"][p]                                # SetWorldPos(mPosGBA)
        else:
            T = sc["xf"][c]
            xc = affine(T["Rcw_before"], T["tcw_before"], pos[p], variant)   # Xc = Rcw*Xw + tcw
            pos[p] = affine(T["Rwc"], T["twc"], xc, variant)                  # Rwc*Xc + twc
        status[p] = 1
    return status, pos


# ---- scenes ----
def _quat(rng, about=None, angle=None):
    if about is None:
        q = rng.normal(size=4)
    else:
        q = np.concatenate([np.sin(angle / 2) * about / np.linalg.norm(about), [np.cos(angle / 2)]])
    return q / np.linalg.norm(q)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _rot(q, v):
    return np.array(sim3_map({"q": q, "t": [0, 0, 0], "s": 1.0}, v), f64)


def sim3(q, t, s):
    S = np.zeros((), SIM3D_DTYPE)
    S["q"], S["t"], S["s"] = q, t, s
    return S


def sim3_inverse(S):
    """g2o::Sim3::inverse() in plain double arithmetic: the caller's algebra, not part of the call."""
    q = np.array(S["q"]) * [-1, -1, -1, 1]
    return sim3(q, _rot(q, -np.array(S["t"]) / S["s"]), 1.0 / S["s"])


def make_scene(seed, nkf=12, K=5, P=64, lengths=None, nlevels=8, bad_points=(), ref="random", level=None, small=True):
    """nkf key frames of which K are corrected (their ranks a random permutation), P points with a transform each and observation
    lists in ascending key-frame order.  lengths: the list length of each point (cycled; default random 0..min(nkf, 9), a few empty).
    small: the correction is a small rotation, shift and scale change, as a loop closure's is; otherwise any similarity.
    ref: "random" | "first" | "last".  level: a fixed ref_level, else random in [0, nlevels)."""
    rng = np.random.RandomState(seed)
    sf = np.ones(16, f32)
    for l in range(1, 16):
        sf[l] = f32(sf[l - 1] * f32(1.2))
    K = min(K, nkf)
    kfs = np.zeros(nkf, KF_DTYPE)
    kfs["Ow_before"] = rng.uniform(-3, 3, (nkf, 3))
    kfs["Ow_after"] = kfs["Ow_before"] + rng.uniform(-0.4, 0.4, (nkf, 3)).astype(f32)
    kfs["rank"] = -1
    kfs["rank"][rng.choice(nkf, K, replace=False)] = rng.permutation(K)
    xf = np.zeros(K, XF_DTYPE)
    for j in range(K):
        q, t = _quat(rng), rng.uniform(-2, 2, 3)
        xf[j]["Siw"] = sim3(q, t, 1.0)
        if small:
            dq = _quat(rng, rng.normal(size=3), rng.uniform(-0.05, 0.05))
            corrected = sim3(_qmul(dq, q), t + rng.uniform(-0.2, 0.2, 3), rng.uniform(0.9, 1.1))
        else:
            corrected = sim3(_quat(rng), rng.uniform(-2, 2, 3), rng.uniform(0.5, 2.0))
        xf[j]["corrected_Swi"] = sim3_inverse(corrected)
    pos = rng.uniform(-6, 6, (P, 3)).astype(f32)
    pos[:, 2] += f32(9)
    off, obs_kf, ref_pos = [0], [], []
    for p in range(P):
        N = int(lengths[p % len(lengths)]) if lengths is not None else int(rng.randint(0, min(nkf, 9) + 1))
        N = min(N, nkf)
        obs_kf += [int(k) for k in sorted(rng.choice(nkf, N, replace=False))]
        off.append(len(obs_kf))
        ref_pos.append(0 if (ref == "first" or N == 0) else N - 1 if ref == "last" else int(rng.randint(N)))
    flags = np.full(P, MP_OBSERVED, np.uint8)
    flags[list(bad_points)] |= MP_BAD
    return {"xf": xf, "kfs": kfs, "keys": np.arange(P, dtype=np.uint64) * np.uint64(5) + np.uint64(11),
            "corr": rng.randint(0, K, P).astype(np.int32), "off": np.array(off, np.int32), "obs_kf": np.array(obs_kf, np.int32),
            "ref_pos": np.array(ref_pos, np.int32),
            "ref_level": (rng.randint(0, nlevels, P) if level is None else np.full(P, level)).astype(np.uint8),
            "sf": sf, "nlevels": nlevels, "pos": pos, "normal": rng.uniform(-1, 1, (P, 3)).astype(f32),
            "min_dist": rng.uniform(0.5, 2, P).astype(f32), "max_dist": rng.uniform(8, 20, P).astype(f32),
            "desc": rng.randint(0, 256, (P, 32)).astype(np.uint8), "flags": flags}


def make_se3_scene(seed, K=7, P=64, mode="mixed", bad_points=()):
    """K key frames with a pose before and an inverse pose after a bundle adjustment, P points.  mode: "set" (every corr -1),
    "move" (none) or "mixed"."""
    rng = np.random.RandomState(seed)
    xf = np.zeros(K, SE3_DTYPE)
    for j in range(K):
        q, t = _quat(rng), rng.uniform(-2, 2, 3)
        Rb = np.array([_rot(q, e) for e in np.eye(3)]).T
        q2 = _qmul(_quat(rng, rng.normal(size=3), rng.uniform(-0.05, 0.05)), q)
        Ra = np.array([_rot(q2, e) for e in np.eye(3)]).T
        ta = t + rng.uniform(-0.2, 0.2, 3)
        xf[j]["Rcw_before"], xf[j]["tcw_before"] = Rb.ravel(), t
        xf[j]["Rwc"], xf[j]["twc"] = Ra.T.ravel(), -Ra.T @ ta
    pos = rng.uniform(-6, 6, (P, 3)).astype(f32)
    pos[:, 2] += f32(9)
    corr = rng.randint(0, K, P).astype(np.int32)
    if mode == "set":
        corr[:] = -1
    elif mode == "mixed":
        corr[rng.uniform(size=P) < 0.4] = -1
    flags = np.full(P, MP_OBSERVED, np.uint8)
    flags[list(bad_points)] |= MP_BAD
    return {"xf": xf, "keys": np.arange(P, dtype=np.uint64) * np.uint64(5) + np.uint64(11), "corr": corr,
            "pos_set": (pos + rng.uniform(-0.3, 0.3, (P, 3))).astype(f32), "pos": pos, "normal": rng.uniform(-1, 1, (P, 3)).astype(f32),
            "min_dist": rng.uniform(0.5, 2, P).astype(f32), "max_dist": rng.uniform(8, 20, P).astype(f32),
            "desc": rng.randint(0, 256, (P, 32)).astype(np.uint8), "flags": flags}


# ---- the guard scene: what it must contain is asserted by tests/test_correct_model.py through guard_counts() ----
# the seed was chosen by running guard_counts() over seeds 0..7 on the CPU and taking the first at which every variant changes an
# output bit (the search is tests/test_correct_model.py::test_guard_seed_search_is_reproducible)
GUARD_SEED = 0


def guard_scene(seed=None):
    """A fused a*b - c*d moves a double by an ulp, which the one rounding to float hides at all but one point in 2^29.  It shows where
    the result cancels: points 7 and 8 lie where Siw of their key frame maps them to the origin -- t is minus the rotated point as
    the unfused arithmetic gives it, so the right answer is +0 and the fused one is the difference of the roundings -- and the
    corrected inverse of these two key frames is a pure scale, which keeps it."""
    sc = make_scene(GUARD_SEED if seed is None else seed, nkf=10, K=6, P=96, bad_points=(5, 40))
    for j, p in ((0, 7), (1, 8)):
        q = sc["xf"][j]["Siw"]["q"].copy()
        r = sim3_map(sim3(q, [0, 0, 0], 1.0), [f64(c) for c in sc["pos"][p]])
        sc["xf"][j]["Siw"] = sim3(q, [-c for c in r], 1.0)
        sc["xf"][j]["corrected_Swi"] = sim3([0, 0, 0, 1], [0, 0, 0], 1.5)
        sc["corr"][p] = j
    return sc


def guard_se3_scene(seed=None):
    return make_se3_scene(GUARD_SEED if seed is None else seed, K=5, P=96, mode="mixed")


def _differ(a, b):
    return sum(bits(x).tobytes() != bits(y).tobytes() for x, y in zip(a[1:], b[1:]))


def guard_counts(sc, se3):
    """variant -> the number of outputs (position, normal, min, max arrays) the wrong implementation changes at least one bit of."""
    good = correct_sim3(sc)
    cnt = {v: _differ(good, correct_sim3(sc, variant=v)) for v in VARIANTS_SIM3}
    cnt["float_accum"] = _differ(correct_se3(se3), correct_se3(se3, variant="float_accum"))
    return cnt
