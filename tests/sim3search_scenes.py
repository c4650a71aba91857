"""Scenes of the SearchBySim3 tests (tests/test_sim3search_model.py on the CPU, tests/test_sim3search_gpu.py on the device).  Every
key frame is a 128 x 128 image with a set of synthetic features; a scene is two sides (camera, features, row of point keys), the
similarity (s12, R12, t12), th, the taken bytes and the store's points.

edge_scene():   direction 0 on the edge of every comparison of the projection, hand-placed.  Key frame 1 sits at the identity, the
                similarity is 2 * [I | 0], so p3Dc2 = 0.5 * Xw exactly; fx = fy = 64, cx = cy = 0.5 of key frame 1 and z = 1 make
                u = 64 * x + 0.5 exact.  Key frame 2 has other intrinsics (80, 80, 10, 10) and the bounds 16..112 x 16..104, so the
                reference's use of key frame 1's intrinsics decides every bound.  Row 2 holds no point.
assoc_scene():  one point whose u differs between Fuse's association and the frame searches'; key frame 2's mnMaxX is the larger.
agree_scene():  the agreement, the distance threshold, the level window, the taken bytes and the resolution of entries, hand-placed
                site by site (both key frames at the identity, s12 = 1: the two images coincide).
pair_scene():   random pairs of n1 and n2 features with a true similarity between them (scale 1.37), for the row shapes at the wave
                and block edges, n1 != n2, rows without a point, and same_scene() for key1 == key2.
`python tests/sim3search_scenes.py` prints the tallies from the model alone, no device."""
import numpy as np

import localmap_scenes as LS
import sim3search_model as M
from loopfuse_scenes import grid, scale_tables
from projtrack_scenes import _fit_factor

f32, f64 = np.float32, np.float64
W = H = 128
SET1, SET2, ROW1, ROW2 = 0x910, 0x911, 0x920, 0x921
SIZES = ((1, 257), (63, 256), (64, 255), (65, 64), (255, 63), (256, 65), (257, 1))
UP, DN = f32(np.inf), f32(-np.inf)


def camera(R, t, fx, fy, cx, cy, bounds=None):
    sf, _ = scale_tables()
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    Ow = np.zeros(3, f32)
    for r in range(3):                                                    # Ow = -Rcw' tcw: one gemm, alpha = -1
        Ow[r] = f32(f64(-1.0) * sum(f64(R[k, r]) * f64(t[k]) for k in range(3)))
    return dict(Rcw=R, tcw=t, Ow=Ow, fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), mbf=f32(0),
                bounds=bounds or (f32(0), f32(W), f32(0), f32(H)), scale_factors=sf, log_scale_factor=f32(np.log(LS.S)),
                viewing_cos_limit=f32(0.5))


def _kps(xy, octave):
    from orbhip import capi
    kps = np.zeros(len(xy), capi.KP_DTYPE)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    kps["size"], kps["angle"], kps["response"], kps["class_id"] = 31, 10, 50, -1
    kps["octave"] = octave
    return kps


def flip(d, bits):
    d = np.array(d, np.uint8)
    for b in bits:
        d[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return d


def _side(key, row_key, cam, kps, desc):
    _, sig = scale_tables()
    return dict(key=key, row_key=row_key, cam=cam, kps=kps, desc=np.ascontiguousarray(desc, np.uint8), gp=grid(), sig=sig)


def _norm(p):
    return f32(np.sqrt((np.asarray(p, f32).astype(f64) ** 2).sum()))


def _scene(sides, rows, s12, R12, t12, th, pts, taken1=None, taken2=None, stale=(), erased=(), ix=None):
    """pts: list of (key, pos, normal, min_dist, max_dist, desc, flags).  stale: keys whose points leave the map after the rows were
    put and whose slots go to new points with the same data; erased: keys that leave and whose slots stay free."""
    keys = np.array([p[0] for p in pts], np.uint64)
    assert len(set(keys.tolist())) == len(keys) and 0 not in keys
    stale, erased = np.array(list(stale), np.uint64), np.array(list(erased), np.uint64)
    return dict(sides=sides, rows=[np.asarray(r, np.uint64) for r in rows], s12=f32(s12), R12=np.asarray(R12, f32), t12=np.asarray(t12, f32),
                th=f32(th), taken1=taken1, taken2=taken2, keys=keys, pos=np.array([p[1] for p in pts], f32).reshape(-1, 3),
                normal=np.array([p[2] for p in pts], f32).reshape(-1, 3), min_dist=np.array([p[3] for p in pts], f32),
                max_dist=np.array([p[4] for p in pts], f32), pdesc=np.array([p[5] for p in pts], np.uint8).reshape(-1, 32),
                flags=np.array([p[6] for p in pts], np.uint8), stale=stale, erased=erased,
                fresh_keys=(np.arange(len(stale), dtype=np.uint64) + np.uint64(1)) * np.uint64(1000003), ix=ix or {})


def fresh_points(sc):
    """The new points: the data of the stale ones under new keys, every one usable."""
    at = [int(np.nonzero(sc["keys"] == k)[0][0]) for k in sc["stale"]]
    a = [sc[name][at] for name in ("pos", "normal", "min_dist", "max_dist", "pdesc")]
    return [sc["fresh_keys"]] + a + [np.ones(len(at), np.uint8)]


def model_store(sc):
    st = M.Store(1 << 16)
    if len(sc["keys"]):
        st.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
    st.erase(sc["stale"])
    st.erase(sc["erased"])
    if len(sc["stale"]):
        st.put(*fresh_points(sc))
    return st


def reused(sc):
    return dict(zip(sc["stale"].tolist(), sc["fresh_keys"].tolist()))


def model(oracle, sc, variant=None, th_high=M.TH_HIGH, taken=True):
    return M.search_by_sim3(oracle, model_store(sc), sc["sides"], sc["rows"], sc["s12"], sc["R12"], sc["t12"], sc["th"], th_high,
                            sc["taken1"] if taken else None, sc["taken2"] if taken else None, variant, reused(sc))


# ---- the edge scene ----
EDGE_BOUNDS = (f32(16), f32(112), f32(16), f32(104))
EDGE_CASES = ("inside", "u_min", "u_min_below", "u_min_above", "u_max", "u_max_below", "u_max_above", "v_min", "v_min_below",
              "v_min_above", "v_max", "v_max_below", "v_max_above", "behind", "z_pzero", "z_nzero_world", "z_nzero", "z_neg_tiny",
              "z_pos_tiny", "z_pos_tiny_axis", "nan", "bad", "key0", "erased", "taken", "near_on", "near_out", "far_on", "far_out",
              "norm", "view", "level_low", "level_high", "quirk_in", "quirk_out")
EDGE_EXPECT = dict(inside=M.ACTIVE, u_min=M.ACTIVE, u_min_below=M.LEFT, u_min_above=M.ACTIVE, u_max=M.RIGHT, u_max_below=M.ACTIVE,
                   u_max_above=M.RIGHT, v_min=M.ACTIVE, v_min_below=M.TOP, v_min_above=M.ACTIVE, v_max=M.BOTTOM, v_max_below=M.ACTIVE,
                   v_max_above=M.BOTTOM, behind=M.BEHIND, z_pzero=M.RIGHT, z_nzero_world=M.RIGHT, z_nzero=M.LEFT, z_neg_tiny=M.BEHIND,
                   z_pos_tiny=M.RIGHT, z_pos_tiny_axis=M.NONFINITE, nan=M.NONFINITE, bad=M.BAD, key0=M.NO_POINT, erased=M.UNKNOWN,
                   taken=M.SKIPPED, near_on=M.ACTIVE, near_out=M.NEAR, far_on=M.ACTIVE, far_out=M.FAR, norm=M.NEAR, view=M.ACTIVE,
                   level_low=M.ACTIVE, level_high=M.ACTIVE, quirk_in=M.ACTIVE, quirk_out=M.LEFT)
TINY = f32(1.4e-45)       # the smallest positive float


def edge_scene():
    rng = np.random.default_rng(211)
    nc = len(EDGE_CASES)
    ix = {c: i for i, c in enumerate(EDGE_CASES)}
    cam1 = camera(np.eye(3), np.zeros(3), 64, 64, 0.5, 0.5)
    cam2 = camera(np.eye(3), np.zeros(3), 80, 80, 10, 10, EDGE_BOUNDS)
    uv = np.array([[24 + 12 * (k % 7), 24 + 14 * (k // 7)] for k in range(nc)], f32)
    for a, (lo, hi), col in (("u", EDGE_BOUNDS[:2], 0), ("v", EDGE_BOUNDS[2:], 1)):
        for case, val, other in ((a + "_min", lo, 40), (a + "_min_below", np.nextafter(lo, DN), 56), (a + "_min_above", np.nextafter(lo, UP), 72),
                                 (a + "_max", hi, 40), (a + "_max_below", np.nextafter(hi, DN), 56), (a + "_max_above", np.nextafter(hi, UP), 72)):
            uv[ix[case], col], uv[ix[case], 1 - col] = val, other
    uv[ix["quirk_in"]] = (100.5, 60.5)        # inside 16..112 with key frame 1's intrinsics; 80 * x + 10 = 135 with key frame 2's
    uv[ix["quirk_out"]] = (10, 60.5)          # 10 < 16 with key frame 1's; 80 * x + 10 = 21.875 with key frame 2's
    pc = np.zeros((nc, 3), f32)               # the point in camera 2: (x, y, 1)
    pc[:, :2] = ((uv.astype(f64) - 0.5) / 64).astype(f32)
    pc[:, 2] = 1
    assert np.array_equal(pc[:, :2].astype(f64) * 64 + 0.5, uv.astype(f64))      # exact, so the device has no freedom either
    mn, mx = np.zeros(nc, f32), np.zeros(nc, f32)
    for on, out, c, side in (("near_on", "near_out", f32(0.8), +1), ("far_on", "far_out", f32(1.2), -1)):
        fit = None
        for shift in range(64):               # along the lattice row until c * m == dist has a solution
            for k in (ix[on], ix[out]):
                pc[k, 0] = f32((f64(uv[ix[on], 0]) + shift * 0.25 - 0.5) / 64)
                pc[k, 1] = pc[ix[on], 1]
            fit = _fit_factor(c, _norm(pc[ix[on]]), side)
            if fit is not None:
                break
        assert fit is not None
        d = _norm(pc[ix[on]])
        if side > 0:
            mn[ix[on]], mn[ix[out]] = fit
            mx[ix[on]] = mx[ix[out]] = d * f32(2)
        else:
            mx[ix[on]], mx[ix[out]] = fit
            mn[ix[on]] = mn[ix[out]] = d / f32(4)
    dist = np.array([_norm(p) for p in pc], f32)
    free = mx == 0
    mn[free], mx[free] = (dist[free] / f32(2)).astype(f32), (dist[free] * f32(2)).astype(f32)
    # |P - Ow2| = |Xw| = 2 * dist3D passes 0.8 * min = 1.2 * dist3D; the norm of the camera point does not
    mn[ix["norm"]], mx[ix["norm"]] = f32(1.5) * dist[ix["norm"]], f32(4) * dist[ix["norm"]]
    mx[ix["level_low"]], mn[ix["level_low"]] = dist[ix["level_low"]] / f32(1.15), dist[ix["level_low"]] / f32(4.6)
    mx[ix["level_high"]], mn[ix["level_high"]] = dist[ix["level_high"]] * f32(1.2 ** 9.5), dist[ix["level_high"]] / f32(1.1)
    normal = (pc.astype(f64) / dist.astype(f64)[:, None]).astype(f32)            # along the ray
    normal[ix["view"]] = (0, 0, -1)           # a viewing-angle test would reject it; the reference has none here
    pos = (pc * f32(2)).astype(f32)           # Xw = 2 * p3Dc2 (exact)
    pos[ix["behind"]] = -pos[ix["behind"]]
    pos[ix["z_pzero"], 2] = 0
    pos[ix["z_nzero_world"], 2] = -0.0        # the gemm sums from +0.0: z is +0.0 all the same
    pos[ix["z_nzero"], 2] = -TINY             # 0.5 * -1.4e-45 rounds (ties to even) to -0.0: passes `< 0.0`, then u = -inf
    pos[ix["z_neg_tiny"], 2] = f32(-2) * TINY  # z = -1.4e-45 < 0.0
    pos[ix["z_pos_tiny"], 2] = f32(2) * TINY  # z = 1.4e-45: invz overflows to +inf, u = +inf
    pos[ix["z_pos_tiny_axis"]] = (0, 0, f32(2) * TINY)   # x = 0 * inf = NaN
    pos[ix["nan"], 1] = np.nan
    assert pos[ix["z_pzero"], 0] > 0 and pos[ix["z_nzero"], 0] > 0 and pos[ix["z_pos_tiny"], 0] > 0
    # key frame 2's features: one where each case projects (clamped into the image), octave 3: inside [level - 1, level] of ratio 2
    octave = np.full(nc, 3)
    octave[ix["level_low"]], octave[ix["level_high"]] = 0, LS.NLEVELS - 1
    octave[ix["far_on"]] = octave[ix["far_out"]] = 0
    kps2 = _kps(np.stack([np.clip(uv[:, 0], 1, W - 1), np.clip(uv[:, 1], 1, H - 1)], 1), octave)
    desc2 = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    kps1 = _kps(rng.uniform(4, W - 4, (nc, 2)), 0)
    desc1 = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    keys = (np.arange(nc, dtype=np.uint64) + np.uint64(1)) * np.uint64(104729)
    pts = [(keys[j], pos[j], normal[j], mn[j], mx[j], flip(desc2[j], rng.integers(0, 256, 6)), 3 if j == ix["bad"] else 1) for j in range(nc)]
    row1 = keys.copy()
    row1[ix["key0"]] = 0
    taken1 = np.zeros(nc, np.uint8)
    taken1[ix["taken"]] = 1
    sides = [_side(SET1, ROW1, cam1, kps1, desc1), _side(SET2, ROW2, cam2, kps2, desc2)]
    return _scene(sides, [row1, np.zeros(nc, np.uint64)], 2.0, np.eye(3), np.zeros(3), 1.5, pts, taken1, None, erased=[keys[ix["erased"]]], ix=ix)


def assoc_scene():
    """Returns (scene, u of the reference's association, u of the frame searches'): key frame 2's mnMaxX is the larger, so exactly
    one of them is inside (u < max_x)."""
    rng = np.random.default_rng(7)
    R1, t1, _ = LS.pose(rng)
    R2, t2, _ = LS.pose(rng)
    R12, t12, _ = LS.pose(rng, 0.003, 0.02)
    cam1 = camera(R1, t1, 0.8 * W, 0.82 * W, W / 2 - 0.5, H / 2 + 0.5)
    kps1 = _kps([[30, 30]], 3)
    d = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    while True:
        Pw = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(1, 8)], f32)
        cam2 = camera(R2, t2, 0.8 * W, 0.82 * W, W / 2 - 0.5, H / 2 + 0.5)
        sides = [_side(SET1, ROW1, cam1, kps1, d[:1]), _side(SET2, ROW2, cam2, _kps([[60, 60]], 3), d[1:])]
        pts = [(np.uint64(424243), Pw, (0, 0, 1), f32(0.01), f32(100), d[1], 1)]
        sc = _scene(sides, [[424243], [0]], 1.37, R12, t12, 3.0, pts)
        st = model_store(sc)
        sR12, sR21, t21 = M.compose(sc["s12"], R12, t12)
        ua = M.direction_queries(st, cam1, sR21, t21, cam1, cam2, 3.0, sc["rows"][0], None)[0]["u"][0]
        ub = M.direction_queries(st, cam1, sR21, t21, cam1, cam2, 3.0, sc["rows"][0], None, "other_assoc")[0]["u"][0]
        if ua != ub and 20 < ua < W - 20:
            break
    cam2["bounds"] = (f32(0), max(ua, ub), f32(0), f32(H))
    q = M.direction_queries(st, cam1, sR21, t21, cam1, cam2, 3.0, sc["rows"][0], None)[0] if ua < ub else \
        M.direction_queries(st, cam1, sR21, t21, cam1, cam2, 3.0, sc["rows"][0], None, "other_assoc")[0]
    sides[1]["kps"] = _kps([[min(ua, ub), q["v"][0]]], int(q["max_level"][0]))
    return sc, ua, ub


# ---- the agreement scene ----
def agree_scene():
    """Sites 24 pixels apart, windows of 3 pixels (th = 3, level 0).  Returns the scene; sc["ix"][name] = (feature of key frame 1,
    feature of key frame 2) of each site, sc["expect"] = match12."""
    rng = np.random.default_rng(223)
    cam = camera(np.eye(3), np.zeros(3), 64, 64, 0.5, 0.5)
    F = ([], [])            # per key frame: (x, y, octave, desc)
    rows = ([], [])
    pts, ix, taken, expect, stale, erased = [], {}, ([], []), {}, [], []
    nextkey = [15485863]

    def feat(kf, x, y, octave=0, desc=None):
        F[kf].append((x, y, octave, rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc))
        rows[kf].append(0)
        return len(F[kf]) - 1

    def point(kf, i, x, y, desc, flags=1):
        pc = np.array([(x - 0.5) / 64, (y - 0.5) / 64, 1], f32)
        d = _norm(pc)
        key = nextkey[0]
        nextkey[0] += 15485863
        pts.append((np.uint64(key), pc, (0, 0, 1), d / f32(2), d / f32(1.1), desc, flags))     # ratio < 1: level 0, levels [-1, 0]
        rows[kf][i] = key
        return key

    def site(k):
        return 16.0 + 24 * (k % 5), 16.0 + 24 * (k // 5)

    def mutual(name, k, d01=5, d10=7, flags1=1):
        x, y = site(k)
        a, b = feat(0, x, y), feat(1, x, y)
        ka = point(0, a, x, y, flip(F[1][b][3], rng.choice(256, d01, replace=False)), flags1)
        point(1, b, x, y, flip(F[0][a][3], rng.choice(256, d10, replace=False)))
        ix[name] = (a, b)
        return a, b, ka

    a, b, _ = mutual("mutual", 0)
    expect[a] = b
    x, y = site(1)                                            # one-sided, direction 0: the best feature holds no point
    a, b = feat(0, x, y), feat(1, x, y)
    point(0, a, x, y, flip(F[1][b][3], (1, 2, 3)))
    ix["only_0"] = (a, b)
    x, y = site(2)                                            # one-sided, direction 1
    a, b = feat(0, x, y), feat(1, x, y)
    point(1, b, x, y, flip(F[0][a][3], (1, 2, 3)))
    ix["only_1"] = (a, b)
    x, y = site(3)                                            # chain: a -> b, b -> a2
    a, a2, b = feat(0, x, y), feat(0, x + 2, y), feat(1, x, y)
    point(0, a, x, y, flip(F[1][b][3], (4, 5)))
    point(1, b, x, y, flip(F[0][a2][3], (6,)))
    ix["chain"] = (a, b)
    x, y = site(4)                                            # a and a2 both name b; b names a
    a, a2, b = feat(0, x, y), feat(0, x + 2, y), feat(1, x, y)
    point(0, a, x, y, flip(F[1][b][3], (4, 5)))
    point(0, a2, x + 2, y, flip(F[1][b][3], (8,)))
    point(1, b, x, y, flip(F[0][a][3], (6,)))
    ix["shared"] = (a, b)
    ix["shared_other"] = (a2, b)
    expect[a] = b
    a, b, _ = mutual("d100", 5, 100, 100)                     # exactly TH_HIGH both ways
    expect[a] = b
    mutual("d101_0", 6, 101, 5)
    mutual("d101_1", 7, 5, 101)
    a, b, _ = mutual("d60", 8, 60, 60)                        # above TH_LOW
    expect[a] = b
    a, b, _ = mutual("taken1", 9)
    taken[0].append(a)
    a, b, _ = mutual("taken2", 10)
    taken[1].append(b)
    x, y = site(11)                                           # levels: b_up on level 1 is nearer than b on level 0
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    a, b, b_up = feat(0, x, y), feat(1, x, y, 0, flip(base, range(30))), feat(1, x + 1, y, 1, base)
    point(0, a, x, y, flip(base, (200, 201)))
    point(1, b, x, y, flip(F[0][a][3], (6,)))
    ix["levels"] = (a, b)
    ix["levels_up"] = (a, b_up)
    expect[a] = b
    mutual("bad", 12, flags1=3)
    _, _, k = mutual("erased", 13)
    erased.append(k)
    _, _, k = mutual("stale", 14)
    stale.append(k)
    n = [len(F[0]), len(F[1])]
    assert n[0] != n[1]
    sides = [_side(key, rk, cam, _kps([(f[0], f[1]) for f in F[s]], [f[2] for f in F[s]]), np.array([f[3] for f in F[s]], np.uint8))
             for s, (key, rk) in enumerate(((SET1, ROW1), (SET2, ROW2)))]
    tk = [np.zeros(n[s], np.uint8) for s in range(2)]
    for s in range(2):
        tk[s][taken[s]] = 1
    sc = _scene(sides, [rows[0], rows[1]], 1.0, np.eye(3), np.zeros(3), 3.0, pts, tk[0], tk[1], stale, erased, ix)
    sc["expect"] = np.array([expect.get(i, -1) for i in range(n[0])], np.int32)
    return sc


# ---- random pairs ----
def pair_scene(n1, n2, seed=5, frac=0.6, empty=(False, False), use_taken=True):
    """Landmarks seen by both key frames: key frame 2's copy of a landmark is key frame 1's carried through the similarity, as the
    two sides of a loop are.  Key frame 2's features lie where KEY FRAME 1's intrinsics put them -- the reference's projection."""
    rng = np.random.default_rng(seed + 1000 * n1 + n2)
    fx, fy, cx, cy = f32(0.8 * W), f32(0.82 * W), f32(W / 2 - 0.5), f32(H / 2 + 0.5)
    R1, t1, _ = LS.pose(rng)
    R2, t2, _ = LS.pose(rng, 0.01, 0.05)
    R12, t12, _ = LS.pose(rng, 0.003, 0.02)
    s12 = f32(1.37)
    cam1, cam2 = camera(R1, t1, fx, fy, cx, cy), camera(R2, t2, fx * f32(1.02), fy * f32(0.97), cx + f32(2), cy - f32(1.5))
    sR12, sR21, t21 = M.compose(s12, R12, t12)
    N = (n1, n2)
    xy = [rng.uniform(4, W - 4, (n, 2)).astype(f32) for n in N]
    octv = [rng.integers(0, LS.NLEVELS, n) for n in N]
    desc = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in N]
    rows = [np.zeros(n, np.uint64) for n in N]
    pts = []
    key = [7919]

    def add(kf, i, Xw, dist, o, d, flags=1):
        k = key[0]
        key[0] += 7919
        mx = f32(dist * f32(1.2) ** (o - 0.5))
        pts.append((np.uint64(k), Xw.astype(f32), (0, 0, 1), f32(0.3) * dist, mx, d, flags))
        rows[kf][i] = k

    def back(cam, pc):
        return cam["Rcw"].astype(f64).T @ (pc - cam["tcw"].astype(f64))

    m = max(1, int(frac * min(n1, n2)))
    at = [rng.permutation(n)[:m] for n in N]
    for j in range(m):
        for _ in range(200):
            u2, v2, z2 = rng.uniform(8, W - 8), rng.uniform(8, H - 8), rng.uniform(2, 6)
            pc2 = np.array([(u2 - f64(cx)) / f64(fx) * z2, (v2 - f64(cy)) / f64(fy) * z2, z2])
            pc1 = sR12.astype(f64) @ pc2 + np.asarray(t12, f64)
            u1, v1 = f64(fx) * pc1[0] / pc1[2] + f64(cx), f64(fy) * pc1[1] / pc1[2] + f64(cy)
            if 8 < u1 < W - 8 and 8 < v1 < H - 8:
                break
        i1, i2 = at[0][j], at[1][j]
        xy[0][i1], xy[1][i2] = (u1, v1), (u2, v2)
        o = int(rng.integers(0, LS.NLEVELS))
        octv[0][i1] = octv[1][i2] = o
        far = rng.random() < 0.15                             # some pairs beyond TH_HIGH in one direction
        add(0, i1, back(cam1, pc1), f32(np.linalg.norm(pc2)), o, flip(desc[1][i2], rng.choice(256, 110 if far else rng.integers(0, 60), replace=False)),
            3 if rng.random() < 0.05 else 1)
        add(1, i2, back(cam2, pc2), f32(np.linalg.norm(pc1)), o, flip(desc[0][i1], rng.choice(256, rng.integers(0, 60), replace=False)))
    for kf, cam in ((0, cam1), (1, cam2)):                    # points of their own: all over and beyond the other image
        free = [i for i in range(N[kf]) if not rows[kf][i]]
        for i in free[:len(free) // 3]:
            pc = np.array([rng.uniform(-1.2, 1.2), rng.uniform(-1.2, 1.2), rng.uniform(-1, 6)])
            add(kf, i, back(cam, pc), f32(rng.uniform(1, 6)), int(rng.integers(0, LS.NLEVELS)), rng.integers(0, 256, 32, dtype=np.uint8))
    for s in range(2):
        if empty[s]:
            rows[s][:] = 0
    tk = [None, None]
    if use_taken:
        tk = [(rng.random(n) < 0.06).astype(np.uint8) for n in N]
    sides = [_side(SET1, ROW1, cam1, _kps(xy[0], octv[0]), desc[0]), _side(SET2, ROW2, cam2, _kps(xy[1], octv[1]), desc[1])]
    return _scene(sides, rows, s12, R12, t12, 7.5, pts, tk[0], tk[1])


def same_scene(n=50, seed=9):
    """key1 == key2: one key frame on both sides, the identity between the cameras."""
    rng = np.random.default_rng(seed)
    R, t, _ = LS.pose(rng)
    cam = camera(R, t, 0.8 * W, 0.82 * W, W / 2 - 0.5, H / 2 + 0.5)
    xy = rng.uniform(8, W - 8, (n, 2)).astype(f32)
    octv = rng.integers(0, LS.NLEVELS, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    row = np.zeros(n, np.uint64)
    pts = []
    for i in np.nonzero(rng.random(n) < 0.6)[0]:
        z = rng.uniform(2, 6)
        pc = np.array([(xy[i, 0] - f64(cam["cx"])) / f64(cam["fx"]) * z, (xy[i, 1] - f64(cam["cy"])) / f64(cam["fy"]) * z, z])
        dist = f32(np.linalg.norm(pc))
        row[i] = 7919 * (int(i) + 1)
        pts.append((np.uint64(row[i]), (cam["Rcw"].astype(f64).T @ (pc - cam["tcw"].astype(f64))).astype(f32), (0, 0, 1), f32(0.3) * dist,
                    f32(dist * f32(1.2) ** (octv[i] - 0.5)), flip(desc[i], rng.choice(256, 9, replace=False)), 1))
    side = _side(SET1, ROW1, cam, _kps(xy, octv), desc)
    return _scene([side, side], [row, row], 1.0, np.eye(3), np.zeros(3), 7.5, pts)


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    scenes = [("edge", edge_scene()), ("assoc", assoc_scene()[0]), ("agree", agree_scene()), ("same", same_scene())]
    scenes += [("pair %d x %d" % s, pair_scene(*s)) for s in SIZES + ((50, 40),)]
    for name, sc in scenes:
        out = model(oracle, sc)
        print(name, "active", out["n_active"].tolist(), "found", out["nfound"], M.tally(out["code"][0]), M.tally(out["code"][1]))
