"""Scenes of the loop-closing search tests (tests/test_loopfuse_model.py on the CPU, tests/test_loopfuse_gpu.py on the device).
Every target is a 128 x 128 key frame with a set of 1 to 50 synthetic features; every camera is the decomposition of a similarity
whose scale is 0.5, 1.37 or 2, so that Rcw = sRcw / scw rounds.

make():         five target records over four sets of different sizes (one set twice, under two similarities and two th); the loop
                points are made by back-projecting the largest set's features through the first camera
                (tests/localmap_scenes.map_points: every exit of the projection loop is taken), several points per feature.  Each
                target but one has a row in the key-frame table that holds some of the list's points, empty entries and entries
                whose point left the map afterwards; the slots of those went to new points, which are in the list.
edge_scene():   every comparison of the projection on its edge, hand-placed (the similarity 2 * [I | 0] decomposes to the identity;
                fx = fy = 64, cx = cy = 0.5 and z = 1 make u = 64 * x + 0.5 exact).
claim_scene():  the sequential claim, hand-placed: two points with the same best feature, a third that then has none, a closed
                feature that would have been the best, a point among the matched ones, two points at the same distance from one
                feature.
`python tests/loopfuse_scenes.py` prints the tallies from the model alone, no device."""
import numpy as np

import localmap_scenes as LS
import loopfuse_model as LM
from projtrack_scenes import _fit_factor

f32, f64 = np.float32, np.float64
W = H = 128
SET_A, SET_B, SET_C, SET_D = 0x810, 0x811, 0x812, 0x813
ROWS = (0x820, 0x821, 0, 0x823, 0x824)        # the targets' rows in the key-frame table; the third target has none
LOOP_ROWS = (0x830, 0x831, 0x832)             # the matched key frame and two covisibles (ComputeSim3's union)
SIZES = (1, 63, 64, 65, 255, 256, 257)
SCALES = (f32(1.37), f32(0.5), f32(2.0), f32(2.0), f32(1.37))


def scale_tables():
    sf = (LS.S ** np.arange(LS.NLEVELS)).astype(f32)
    return sf, (f32(1.0) / (sf * sf)).astype(f32)


def grid():
    from orbhip import guided
    return guided.grid_params(0, W, 0, H)


def camera_of(Scw, bounds=None, fx=None, fy=None, cx=None, cy=None):
    sf, _ = scale_tables()
    Rcw, tcw, Ow, _ = LM.decompose_sim3(Scw)
    return dict(Rcw=Rcw, tcw=tcw, Ow=Ow, fx=f32(0.8 * W) if fx is None else fx, fy=f32(0.82 * W) if fy is None else fy,
                cx=f32(W / 2 - 0.5) if cx is None else cx, cy=f32(H / 2 + 0.5) if cy is None else cy, mbf=f32(0),
                bounds=bounds or (f32(0), f32(W), f32(0), f32(H)), scale_factors=sf, log_scale_factor=f32(np.log(LS.S)),
                viewing_cos_limit=f32(0.5))


def features(rng, n):
    from orbhip import capi
    kps = np.zeros(n, capi.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(4, W - 4, n).astype(f32), rng.uniform(4, H - 4, n).astype(f32)
    kps["size"], kps["angle"], kps["response"], kps["class_id"] = 31, rng.uniform(0, 360, n).astype(f32), 50, -1
    kps["octave"] = rng.integers(0, LS.NLEVELS, n)
    return kps, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def make(seed=29, npoints=300):
    rng = np.random.default_rng(seed)
    sf, sig = scale_tables()
    kA, dA = features(rng, 50)
    # features 40..49 are twins of features 0..9, three pixels (at the feature's scale) to the side: inside the window of a point
    # on the first, outside what a chi-square gate would let through (9 > 5.99)
    for j in range(10):
        kA[40 + j] = kA[j]
        kA["x"][40 + j] = kA["x"][j] + f32(3.0) * sf[kA["octave"][j]] * (f32(1) if kA["x"][j] < W / 2 else f32(-1))
    R, t, _ = LS.pose(rng)
    poses = [(R, t)]
    for ang, shift in ((0.0004, 0.002), (0.001, 0.004), (0.0004, 0.002), (0.0006, 0.003)):
        dR, dt, _ = LS.pose(rng, ang, shift)
        poses.append(((dR.astype(f64) @ R.astype(f64)).astype(f32), (dR.astype(f64) @ t.astype(f64) + dt.astype(f64)).astype(f32)))
    cams = [camera_of(LM.sim3(s, Rk, tk)) for s, (Rk, tk) in zip(SCALES, poses)]
    assert all((c["Rcw"].astype(f64) * f64(s) != LM.sim3(s, Rk, tk)[:3, :3].astype(f64)).any() for c, s, (Rk, tk) in zip(cams, SCALES, poses)
               if s == f32(1.37))         # the division rounded
    ths = [f32(4.0), f32(4.0), f32(4.0), f32(6.0), f32(3.0)]
    gp = grid()
    pts = LS.map_points(rng, cams[0], kA, dA, npoints, W, H)
    for j in range(10):                  # the twin looks like the points made from the first, which itself is 40 bits off now
        dA[40 + j] = dA[j]
        for b in rng.choice(256, 40, replace=False):
            dA[j, b >> 3] ^= np.uint8(1 << (b & 7))
    sets = {SET_A: (kA, dA), SET_B: (kA[:33].copy(), dA[:33].copy()), SET_C: (kA[7:8].copy(), dA[7:8].copy()),
            SET_D: (kA[::3].copy(), dA[::3].copy())}
    targets = [dict(key=k, cam=c, th=th, kps=sets[k][0], desc=sets[k][1], gp=gp, u_right=None, sig=sig)
               for k, c, th in zip((SET_A, SET_B, SET_C, SET_A, SET_D), cams, ths)]
    # the points that leave the map after the rows were put, and the new points whose slots those were
    stale = np.sort(rng.choice(npoints, 24, replace=False))
    fresh_keys = (np.arange(len(stale), dtype=np.uint64) + np.uint64(1)) * np.uint64(1000003)
    # the loop list: every point (the stale ones with the key the store forgot), the new points, a few NULLs
    order = rng.permutation(npoints + len(stale) + 6)
    pool = np.concatenate([pts["keys"], fresh_keys, np.zeros(6, np.uint64)])
    loop = pool[order]
    # the targets' rows: a tenth of the list each, NULLs, and stale entries; different lengths, one over a block of 256
    rows = {}
    for k, (row_key, length) in enumerate(zip(ROWS, (40, 300, 0, 65, 257))):
        if not row_key:
            continue
        pick = rng.choice(npoints, min(length, npoints) * 2 // 3, replace=False)
        row = np.zeros(length, np.uint64)
        row[rng.choice(length, len(pick), replace=False)] = pts["keys"][pick]
        rows[row_key] = row
    rows[ROWS[0]][:8] = 0
    rows[ROWS[0]][:4] = pts["keys"][stale[:4]]          # stale entries in a row whose target sees the list's new points
    rows[ROWS[0]] = _dedup(rows[ROWS[0]])
    # ComputeSim3's union: three overlapping rows over the points
    k = pts["keys"]
    loop_rows = {LOOP_ROWS[0]: k[:130].copy(), LOOP_ROWS[1]: k[90:240][::-1].copy(), LOOP_ROWS[2]: np.concatenate([k[200:], np.zeros(5, np.uint64)])}
    # vpMatched of target 0: a fifth of its features hold a point already, most of them points of the union
    matched = np.zeros(len(kA), np.uint64)
    feat = rng.choice(len(kA), 10, replace=False)
    matched[feat] = k[rng.choice(npoints, 10, replace=False)]
    return dict(targets=targets, sets=sets, loop=loop, rows=rows, loop_rows=loop_rows, matched=matched, stale=stale, fresh_keys=fresh_keys,
                **pts)


def _dedup(row):
    seen, out = set(), row.copy()
    for i, k in enumerate(row):
        if int(k) and int(k) in seen:
            out[i] = 0
        seen.add(int(k))
    return out


def fresh_points(sc):
    """The new points: the data of the stale ones under new keys, every one usable."""
    a = [sc[name][sc["stale"]] for name in ("pos", "normal", "min_dist", "max_dist", "pdesc")]
    return [sc["fresh_keys"]] + a + [np.ones(len(sc["stale"]), np.uint8)]


def model_store(sc):
    st = LM.Store(1 << 16)
    st.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
    if len(sc.get("stale", ())):
        st.erase(sc["keys"][sc["stale"]])
        st.put(*fresh_points(sc))
    return st


def target_rows(sc):
    return [sc["rows"].get(r) if r else None for r in (sc.get("row_keys") or ROWS)[:len(sc["targets"])]]


# ---- the edge scene ----
EDGE_BOUNDS = (f32(16), f32(112), f32(16), f32(104))
EDGE_CASES = ("inside", "u_min", "u_min_below", "u_min_above", "u_max", "u_max_below", "u_max_above", "v_min", "v_min_below",
              "v_min_above", "v_max", "v_max_below", "v_max_above", "behind", "z_zero", "nan", "bad", "key0", "unknown", "held",
              "near_on", "near_out", "far_on", "far_out", "view_on", "view_out", "level_low", "level_high")
EDGE_EXPECT = dict(inside=LM.ACTIVE, u_min=LM.ACTIVE, u_min_below=LM.FM.LEFT, u_min_above=LM.ACTIVE, u_max=LM.FM.RIGHT,
                   u_max_below=LM.ACTIVE, u_max_above=LM.FM.RIGHT, v_min=LM.ACTIVE, v_min_below=LM.FM.TOP, v_min_above=LM.ACTIVE,
                   v_max=LM.FM.BOTTOM, v_max_below=LM.ACTIVE, v_max_above=LM.FM.BOTTOM, behind=LM.FM.BEHIND, z_zero=None,
                   nan=LM.FM.NONFINITE, bad=LM.BAD, key0=LM.NO_POINT, unknown=LM.UNKNOWN, held=LM.SKIPPED, near_on=LM.ACTIVE,
                   near_out=LM.FM.NEAR, far_on=LM.ACTIVE, far_out=LM.FM.FAR, view_on=LM.ACTIVE, view_out=LM.FM.VIEW,
                   level_low=LM.ACTIVE, level_high=LM.ACTIVE)


def edge_scene():
    from orbhip import capi
    rng = np.random.default_rng(107)
    nc = len(EDGE_CASES)
    ix = {c: i for i, c in enumerate(EDGE_CASES)}
    sf, sig = scale_tables()
    cam = camera_of(LM.sim3(2.0, np.eye(3), np.zeros(3)), EDGE_BOUNDS, f32(64), f32(64), f32(0.5), f32(0.5))
    assert np.array_equal(cam["Rcw"], np.eye(3, dtype=f32)) and not cam["tcw"].any() and not cam["Ow"].any()
    uv = np.array([[24 + 12 * (k % 7), 24 + 16 * (k // 7)] for k in range(nc)], f32)
    up, dn = f32(np.inf), f32(-np.inf)
    for a, (lo, hi), col in (("u", EDGE_BOUNDS[:2], 0), ("v", EDGE_BOUNDS[2:], 1)):
        for case, val, other in ((a + "_min", lo, 40), (a + "_min_below", np.nextafter(lo, dn), 56), (a + "_min_above", np.nextafter(lo, up), 72),
                                 (a + "_max", hi, 40), (a + "_max_below", np.nextafter(hi, dn), 56), (a + "_max_above", np.nextafter(hi, up), 72)):
            uv[ix[case], col], uv[ix[case], 1 - col] = val, other
    pos = np.zeros((nc, 3), f32)
    pos[:, :2] = ((uv.astype(f64) - 0.5) / 64).astype(f32)
    pos[:, 2] = 1
    assert np.array_equal(pos[:, :2].astype(f64) * 64 + 0.5, uv.astype(f64))      # exact, so the device has no freedom either

    def norm(p):
        return f32(np.sqrt((p.astype(f64) ** 2).sum()))

    mn, mx = np.zeros(nc, f32), np.zeros(nc, f32)
    for on, out, c, side in (("near_on", "near_out", f32(0.8), +1), ("far_on", "far_out", f32(1.2), -1)):
        fit = None
        for shift in range(64):          # along the lattice row until c * m == dist has a solution
            for k in (ix[on], ix[out]):
                pos[k, 0] = f32((f64(uv[ix[on], 0]) + shift * 0.25 - 0.5) / 64)
                pos[k, 1] = pos[ix[on], 1]
            fit = _fit_factor(c, norm(pos[ix[on]]), side)
            if fit is not None:
                break
        assert fit is not None
        d = norm(pos[ix[on]])
        if side > 0:
            mn[ix[on]], mn[ix[out]] = fit
            mx[ix[on]] = mx[ix[out]] = d * f32(2)
        else:
            mx[ix[on]], mx[ix[out]] = fit
            mn[ix[on]] = mn[ix[out]] = d / f32(4)
    dist = np.array([norm(p) for p in pos], f32)
    free = mx == 0
    mn[free], mx[free] = (dist[free] / f32(2)).astype(f32), (dist[free] * f32(2)).astype(f32)
    normal = (pos.astype(f64) / dist.astype(f64)[:, None]).astype(f32)     # along the ray: the bounds' cases lie far off the axis
    normal[ix["view_on"]] = normal[ix["view_out"]] = (0, 0, 0)
    normal[ix["view_on"], 2] = f32(0.5) * dist[ix["view_on"]]             # PO . n = 1 * nz: exactly 0.5 * dist3D
    normal[ix["view_out"], 2] = np.nextafter(f32(0.5) * dist[ix["view_out"]], dn)
    mx[ix["level_low"]], mn[ix["level_low"]] = dist[ix["level_low"]] / f32(1.15), dist[ix["level_low"]] / f32(4.6)
    mx[ix["level_high"]], mn[ix["level_high"]] = dist[ix["level_high"]] * f32(1.2 ** 9.5), dist[ix["level_high"]] / f32(1.1)
    pos[ix["behind"]] = -pos[ix["behind"]]
    pos[ix["z_zero"], 2] = 0
    pos[ix["nan"], 1] = np.nan
    # the target's features: one where each case projects (clamped into the image), octave 3: inside [level - 1, level] of ratio 2
    kps = np.zeros(nc, capi.KP_DTYPE)
    kps["x"], kps["y"] = np.clip(uv[:, 0], 1, W - 1), np.clip(uv[:, 1], 1, H - 1)
    kps["size"], kps["angle"], kps["response"], kps["octave"], kps["class_id"] = 31, 10, 50, 3, -1
    kps["octave"][ix["level_low"]], kps["octave"][ix["level_high"]] = 0, LS.NLEVELS - 1
    kps["octave"][ix["far_on"]] = kps["octave"][ix["far_out"]] = 0
    desc = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    pdesc = desc.copy()
    for j in range(nc):
        for b in rng.integers(0, 256, 6):
            pdesc[j, b >> 3] ^= np.uint8(1 << (b & 7))
    flags = np.ones(nc, np.uint8)
    flags[ix["bad"]] |= 2
    keys = (np.arange(nc, dtype=np.uint64) + np.uint64(1)) * np.uint64(104729)
    loop = keys.copy()
    loop[ix["key0"]] = 0
    loop[ix["unknown"]] = 777777                                          # a key the store never had
    row = np.array([keys[ix["held"]], 0, keys[ix["bad"]]], np.uint64)     # (the bad point is held by nobody: GetMapPoints leaves it out)
    target = dict(key=SET_A, cam=cam, th=f32(1.5), kps=kps, desc=desc, gp=grid(), u_right=None, sig=sig)
    return dict(targets=[target], sets={SET_A: (kps, desc)}, loop=loop, rows={ROWS[0]: row}, row_keys=(ROWS[0],), keys=keys, pos=pos,
                normal=normal, min_dist=mn, max_dist=mx, pdesc=pdesc, flags=flags, ix=ix, stale=np.zeros(0, np.int64),
                fresh_keys=np.zeros(0, np.uint64))


# ---- the claim scene ----
CLAIM_POINTS = ("first", "second", "third", "closed_best", "matched", "tie_a", "tie_b")


def claim_scene():
    """Features 0, 1: two pixels apart, the points first / second / third all project onto feature 0.  Feature 2 is closed and holds
    `matched`; feature 3 is three pixels from it.  Feature 4 stands alone; tie_a and tie_b are equally far from it."""
    from orbhip import capi
    rng = np.random.default_rng(109)
    sf, sig = scale_tables()
    cam = camera_of(LM.sim3(0.5, np.eye(3), np.zeros(3)), None, f32(64), f32(64), f32(0.5), f32(0.5))
    fxy = np.array([[30, 30], [32, 30], [80, 30], [83, 30], [50, 90]], f32)
    kps = np.zeros(len(fxy), capi.KP_DTYPE)
    kps["x"], kps["y"] = fxy[:, 0], fxy[:, 1]
    kps["size"], kps["angle"], kps["response"], kps["octave"], kps["class_id"] = 31, 10, 50, 3, -1
    desc = rng.integers(0, 256, (len(fxy), 32), dtype=np.uint8)

    def flipped(d, bits):
        d = d.copy()
        for b in bits:
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    desc[1] = flipped(desc[0], range(0, 12))                              # 12 bits from feature 0
    desc[3] = flipped(desc[2], range(0, 20))
    ix = {c: i for i, c in enumerate(CLAIM_POINTS)}
    at = {"first": 0, "second": 0, "third": 0, "closed_best": 2, "matched": 2, "tie_a": 4, "tie_b": 4}
    pdesc = np.zeros((len(CLAIM_POINTS), 32), np.uint8)
    pdesc[ix["first"]] = desc[0]                                          # 0 from feature 0, 12 from feature 1
    pdesc[ix["second"]] = flipped(desc[0], (100, 101, 102))               # 3 from feature 0, 15 from feature 1
    pdesc[ix["third"]] = flipped(desc[0], (200,))
    pdesc[ix["closed_best"]] = desc[2]                                    # 0 from the closed feature 2, 20 from feature 3
    pdesc[ix["matched"]] = desc[2]
    pdesc[ix["tie_a"]] = pdesc[ix["tie_b"]] = flipped(desc[4], (7, 9))
    uv = np.array([fxy[at[c]] for c in CLAIM_POINTS], f32)
    pos = np.zeros((len(CLAIM_POINTS), 3), f32)
    pos[:, :2] = ((uv.astype(f64) - 0.5) / 64).astype(f32)
    pos[:, 2] = 1
    dist = np.sqrt((pos.astype(f64) ** 2).sum(axis=1)).astype(f32)
    keys = (np.arange(len(CLAIM_POINTS), dtype=np.uint64) + np.uint64(1)) * np.uint64(15485863)
    matched = np.zeros(len(fxy), np.uint64)
    matched[2] = keys[ix["matched"]]
    target = dict(key=SET_A, cam=cam, th=f32(2.0), kps=kps, desc=desc, gp=grid(), u_right=None, sig=sig)
    return dict(targets=[target], sets={SET_A: (kps, desc)}, loop=keys.copy(), rows={}, row_keys=(0,),
                loop_rows={LOOP_ROWS[0]: keys[:3].copy(), LOOP_ROWS[1]: keys[2:].copy()}, matched=matched, keys=keys, pos=pos,
                normal=np.tile(np.array([0, 0, 1], f32), (len(keys), 1)), min_dist=(dist / f32(2)).astype(f32),
                max_dist=(dist * f32(2)).astype(f32), pdesc=pdesc, flags=np.ones(len(keys), np.uint8), ix=ix,
                stale=np.zeros(0, np.int64), fresh_keys=np.zeros(0, np.uint64))


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    for name, sc in (("main", make()), ("edge", edge_scene()), ("claim", claim_scene())):
        st = model_store(sc)
        for k, (q, code, qd, na, bi, bd) in enumerate(LM.fuse_sim3(oracle, st, sc["targets"], target_rows(sc), sc["loop"])):
            print(name, k, len(sc["targets"][k]["kps"]), "features", len(sc["loop"]), "points; active", na, "<= TH_LOW",
                  int((bd <= LM.TH_LOW).sum()), LM.tally(code))
        if "loop_rows" in sc:
            keys, q, code, qd, na, nm, match = LM.search_loop_points(oracle, st, sc["targets"][0], list(sc["loop_rows"].values()), sc["matched"])
            print(name, "loop points", len(keys), "active", na, "matches", nm, LM.tally(code))
