"""Independent numpy model of orbhip_map_refresh (include/orbhip.h): MapPoint::ComputeDistinctiveDescriptors
(ref: src/MapPoint.cc:257-322) and MapPoint::UpdateNormalAndDepth (ref: :345-386) from a point's observation list, written from the
reference and the arithmetic docs/parity.md fixes ("UpdateNormalAndDepth"), with np.float32 / np.float64 scalars: every operation is
one individually rounded IEEE operation.  The `variant` arguments compute what a wrong implementation would, for the guard scenes
that tests/test_refresh_model.py asserts to discriminate.  No device, no liborbhip."""
import numpy as np

f32, f64 = np.float32, np.float64
REFRESH_DESC, REFRESH_NORMAL, KF_BAD, MP_OBSERVED, MP_BAD = 1, 2, 1, 1, 2
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])   # cv::KeyPoint / orbhip_keypoint
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def bits(a):
    """Bit patterns of float32 values: what the tests compare."""
    return np.ascontiguousarray(a, f32).view(np.uint32)


def hamming_matrix(rows):
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    return _POP[rows[:, None, :] ^ rows[None, :, :]].sum(axis=2)


def distinctive(rows, bad, variant=None):
    """rows [N][32], bad [N] -> the list position of the winning descriptor, or -1 when every observer is bad.
    variant: "last" = the last row of least median wins; "upper" = the upper middle of an even row; "keep_bad" = bad observers vote."""
    keep = [i for i in range(len(rows)) if variant == "keep_bad" or not bad[i]]
    if not keep:
        return -1
    D = hamming_matrix(np.asarray(rows)[keep])
    N = len(keep)
    k = int(0.5 * (N - 1))
    if variant == "upper":
        k = N // 2
    best, best_median = -1, 0x7FFFFFFF
    for i in range(N):
        median = int(np.sort(D[i])[k])
        if median < best_median or (variant == "last" and median == best_median):
            best_median, best = median, i
    return keep[best]


def norm3(d, variant=None):
    """cv::norm(NORM_L2) of a CV_32F 3-vector: squares accumulated in double, the root in double."""
    if variant == "float_norm":
        s = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
        return f64(np.sqrt(s))
    s = (f64(d[0]) * f64(d[0]) + f64(d[1]) * f64(d[1])) + f64(d[2]) * f64(d[2])
    return np.sqrt(f64(s))


def normal_depth(pos, Ows, ref, level, sf, nlevels, variant=None):
    """pos [3], Ows [N][3] in list order, ref = position of mpRefKF in the list, level = octave of its feature.
    Returns (normal [3] f32, min_dist f32, max_dist f32).  variant: "descending" | "float_norm" | "divide"."""
    pos, Ows = np.asarray(pos, f32), np.asarray(Ows, f32).reshape(-1, 3)
    n = len(Ows)
    normal = [f32(0), f32(0), f32(0)]
    order = range(n - 1, -1, -1) if variant == "descending" else range(n)
    with np.errstate(all="ignore"):
        for i in order:
            d = [f32(pos[c] - Ows[i][c]) for c in range(3)]
            nrm = norm3(d, variant)
            if variant == "divide":
                t = [f32(d[c] / f32(nrm)) for c in range(3)]
            else:
                a = f32(f64(1.0) / nrm)                                  # a MatExpr scaled by alpha = 1.0 / norm
                t = [f32(d[c] * a) for c in range(3)]
            normal = [f32(t[c] + normal[c]) for c in range(3)]           # scaleAdd on CV_32F
        inv = f32(f64(1.0) / f64(n))
        normal = [f32(normal[c] * inv) for c in range(3)]                # convertTo with a float scale
        d = [f32(pos[c] - Ows[ref][c]) for c in range(3)]
        dist = f32(norm3(d))
        mx = f32(dist * f32(sf[level]))
        mn = f32(mx / f32(sf[nlevels - 1]))
    return np.array(normal, f32), mn, mx


def refresh(sc, what, store=None):
    """The whole call over the scene `sc` (make_scene) on `store` (default: the scene's initial values; a dict of pos, normal, min_dist,
    max_dist, desc, flags by point index).  Returns (status, best_pos, desc, normal, min_dist, max_dist) as the call does; store is
    not modified."""
    st = store or sc
    P = len(sc["keys"])
    status, best = np.zeros(P, np.uint8), np.full(P, -1, np.int32)
    desc, normal = st["desc"].copy(), np.array(st["normal"], f32).copy()
    mn, mx = np.array(st["min_dist"], f32).copy(), np.array(st["max_dist"], f32).copy()
    for p in range(P):
        a, b = sc["off"][p], sc["off"][p + 1]
        if (st["flags"][p] & MP_BAD) or b == a:
            continue
        kf, idx = sc["obs_kf"][a:b], sc["obs_idx"][a:b]
        if what & REFRESH_DESC:
            rows = [sc["sets"][k][1][i] for k, i in zip(kf, idx)]
            w = distinctive(rows, [sc["kf_flags"][k] & KF_BAD for k in kf])
            if w >= 0:
                best[p], desc[p], status[p] = w, rows[w], status[p] | REFRESH_DESC
        if what & REFRESH_NORMAL:
            r = sc["ref_pos"][p]
            level = int(sc["sets"][kf[r]][0]["octave"][idx[r]])
            normal[p], mn[p], mx[p] = normal_depth(st["pos"][p], sc["Ow"][kf], r, level, sc["sf"], sc["nlevels"])
            status[p] |= REFRESH_NORMAL
    return status, best, desc, normal, mn, mx


def make_scene(seed, nkf=20, P=64, lengths=None, nfeat=(8, 64), nlevels=8, bad_kfs=(), bad_points=(), octave=None, flip=5,
               coarse=False, ref="random"):
    """nkf key frames with small feature sets and camera centres, P points with observation lists in ascending key-frame order.
    lengths: the list length of each point (cycled; default random 1..min(nkf, 9)).  The observers' descriptors of a point are its
    own descriptor with `flip` random bits flipped, so equal medians happen.  coarse: positions and centres on a coarse grid (few
    mantissa bits), which makes rounding differences rare -- the opposite is wanted, so the default draws full-precision values.
    ref: "random" | "first" | "last".  octave: a fixed octave for every feature, else random in [0, nlevels)."""
    rng = np.random.RandomState(seed)
    sf = np.ones(16, f32)
    for l in range(1, 16):
        sf[l] = f32(sf[l - 1] * f32(1.2))
    sets, Ow = [], np.zeros((nkf, 3), f32)
    for k in range(nkf):
        n = int(rng.randint(nfeat[0], nfeat[1] + 1))
        kps = np.zeros(n, KP_DTYPE)
        kps["x"], kps["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        kps["octave"] = rng.randint(0, nlevels, n) if octave is None else octave
        kps["size"], kps["class_id"] = 31, -1
        sets.append((kps, rng.randint(0, 256, (n, 32)).astype(np.uint8)))
        Ow[k] = rng.uniform(-3, 3, 3)
    if coarse:
        Ow = np.round(Ow * 4) / 4
    pos = rng.uniform(-6, 6, (P, 3)).astype(f32)
    pos[:, 2] += f32(9)
    if coarse:
        pos = (np.round(pos * 4) / 4).astype(f32)
    pdesc = rng.randint(0, 256, (P, 32)).astype(np.uint8)
    used = [set() for _ in range(nkf)]
    off, obs_kf, obs_idx, ref_pos = [0], [], [], []
    for p in range(P):
        N = int(lengths[p % len(lengths)]) if lengths is not None else int(rng.randint(1, min(nkf, 9) + 1))
        N = min(N, nkf)
        for k in sorted(rng.choice(nkf, N, replace=False)):
            free = [i for i in range(len(sets[k][0])) if i not in used[k]]
            i = int(free[rng.randint(len(free))]) if free else int(rng.randint(len(sets[k][0])))
            used[k].add(i)
            if free:   # the feature becomes this point's observation: the point's descriptor with a few bits flipped
                d = pdesc[p].copy()
                for _ in range(int(rng.randint(0, flip + 1))):
                    d[rng.randint(32)] ^= np.uint8(1 << rng.randint(8))
                sets[k][1][i] = d
            obs_kf.append(int(k)), obs_idx.append(i)
        off.append(len(obs_kf))
        ref_pos.append(0 if (ref == "first" or N == 0) else N - 1 if ref == "last" else int(rng.randint(N)))
    kf_flags = np.zeros(nkf, np.uint32)
    kf_flags[list(bad_kfs)] = KF_BAD
    flags = np.full(P, MP_OBSERVED, np.uint8)
    flags[list(bad_points)] |= MP_BAD
    return {"sets": sets, "Ow": Ow.astype(f32), "kf_flags": kf_flags, "set_keys": np.arange(nkf, dtype=np.uint64) + np.uint64(0x5000),
            "keys": np.arange(P, dtype=np.uint64) * np.uint64(3) + np.uint64(7), "pos": pos,
            "normal": rng.uniform(-1, 1, (P, 3)).astype(f32), "min_dist": rng.uniform(0.5, 2, P).astype(f32),
            "max_dist": rng.uniform(8, 20, P).astype(f32), "desc": pdesc, "flags": flags,
            "off": np.array(off, np.int32), "obs_kf": np.array(obs_kf, np.int32), "obs_idx": np.array(obs_idx, np.int32),
            "ref_pos": np.array(ref_pos, np.int32), "sf": sf, "nlevels": nlevels}


# ---- the guard scenes: what each must contain is asserted by tests/test_refresh_model.py through guard_counts() ----
# the seed was chosen by running guard_counts() over seeds 0..7 on the CPU (every one of them discriminates); two bad key frames
GUARD_SEED, GUARD_BAD_KFS = 3, (2, 7)


def guard_scene():
    return make_scene(GUARD_SEED, nkf=12, P=96, bad_kfs=GUARD_BAD_KFS, flip=3)


def _lists(sc, p):
    a, b = sc["off"][p], sc["off"][p + 1]
    kf, idx = sc["obs_kf"][a:b], sc["obs_idx"][a:b]
    rows = [sc["sets"][k][1][i] for k, i in zip(kf, idx)]
    bad = [int(sc["kf_flags"][k] & KF_BAD) for k in kf]
    return kf, idx, rows, bad


def guard_counts(sc):
    """For each property (a) .. (g): the number of points of the scene at which the wrong implementation gives another result."""
    cnt = dict.fromkeys("abcdefg", 0)
    for p in range(len(sc["keys"])):
        if sc["off"][p + 1] == sc["off"][p] or (sc["flags"][p] & MP_BAD):
            continue
        kf, idx, rows, bad = _lists(sc, p)
        r = sc["ref_pos"][p]
        level = int(sc["sets"][kf[r]][0]["octave"][idx[r]])
        args = (sc["pos"][p], sc["Ow"][kf], r, level, sc["sf"], sc["nlevels"])
        good = normal_depth(*args)
        for name, variant in (("a", "descending"), ("b", "float_norm"), ("c", "divide")):
            other = normal_depth(*args, variant=variant)
            cnt[name] += bits(good[0]).tobytes() != bits(other[0]).tobytes()
        w = distinctive(rows, bad)
        cnt["d"] += w != distinctive(rows, bad, "last")
        cnt["e"] += (len(rows) - sum(bad)) % 2 == 0 and w != distinctive(rows, bad, "upper")
        wb = distinctive(rows, bad, "keep_bad")
        cnt["f"] += wb >= 0 and bad[wb] == 1
        if any(bad) and not all(bad):
            keep = [i for i in range(len(rows)) if not bad[i]]
            other = normal_depth(sc["pos"][p], sc["Ow"][kf[keep]], 0, level, sc["sf"], sc["nlevels"])
            cnt["g"] += bits(good[0]).tobytes() != bits(other[0]).tobytes()
    return cnt
