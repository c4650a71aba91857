"""Scenes of the projection-tracking tests: 376 x 241 frames of the synthetic stream with a few hundred features.  The current
frame is frame 0; the source frame (the last frame, or the key frame) is frame 1, and its map points are made by back-projecting
its key points through the current camera (tests/localmap_scenes.map_points), so that every rejection rule of both loops is taken.
Seeds are chosen so that tests/test_projtrack_model.py's floors hold; `python tests/projtrack_scenes.py` prints the tallies."""
import numpy as np

import localmap_model as LM
import localmap_scenes as LS
import projtrack_model as PM

f32, f64 = np.float32, np.float64
W, H = 376, 241
# name: (mbf, seed, th, th_high)
SCENES = {"mono": (0.0, 3, 15.0, 100), "stereo": (40.0, 5, 7.0, 100)}
CUR, SRC, KFROW = 0x100, 0x101, 0x200


def make(oracle, name, nfeatures=600):
    from orbhip import guided, synth
    mbf, seed, th, th_high = SCENES[name]
    rng = np.random.default_rng(seed)
    frames = synth.make_frames(seed, W, H, 2)
    ref = oracle.Extractor(nfeatures)
    (kA, dA), (kB, dB) = ref(frames[0]), ref(frames[1])
    sf = (LS.S ** np.arange(LS.NLEVELS)).astype(f32)
    R, t, Ow = LS.pose(rng)
    cam = dict(Rcw=R, tcw=t, Ow=Ow, fx=f32(0.8 * W), fy=f32(0.82 * W), cx=f32(W / 2 - 0.5), cy=f32(H / 2 + 0.5), mbf=f32(mbf),
               bounds=(f32(0), f32(W), f32(0), f32(H)), scale_factors=sf, log_scale_factor=f32(np.log(LS.S)), viewing_cos_limit=f32(0.5))
    nB = len(kB)
    pts = LS.map_points(rng, cam, kB, dB, nB, W, H)
    src_kps = kB.copy()
    turned = rng.random(nB) < 0.08           # source angles that disagree with the frame's: the rotation check removes their matches
    src_kps["angle"][turned] = (src_kps["angle"][turned] + rng.uniform(40, 320, int(turned.sum())).astype(f32)) % f32(360)
    n = len(kA)
    sc = dict(name=name, th=f32(th), th_high=th_high, kps=kA, desc=dA, gp=guided.grid_params(0, W, 0, H), cam=cam, src_kps=src_kps,
              src_desc=dB, **pts)
    sc["occupied"] = (rng.random(n) < 0.1).astype(np.uint8)
    sc["u_right"] = None
    if mbf:
        ur = kA["x"] - f32(mbf) / rng.uniform(1, 8, n).astype(f32)
        sc["u_right"] = np.where(rng.random(n) < 0.7, ur, f32(-1)).astype(f32)
    # what the source frame holds per feature: 8 % nothing, 4 % a point that never reaches the store (last-frame form only)
    hold = sc["keys"].copy()
    r = rng.random(nB)
    hold[r < 0.08] = 0
    sc["unknown"] = (r >= 0.08) & (r < 0.12)
    sc["hold"] = hold
    sc["found"] = hold[(r >= 0.5) & (r < 0.56)]          # sAlreadyFound of the key-frame form
    return sc


def stored(sc, last_frame):
    """Indices of the points that go into the store: the last-frame form leaves the `unknown` ones out, the key-frame form
    cannot hold a point the store does not know, so its row has nothing there."""
    return np.nonzero(~sc["unknown"])[0] if last_frame else np.arange(len(sc["keys"]))


def row_keys(sc):
    row = sc["hold"].copy()
    row[sc["unknown"]] = 0
    return row


def model_store(sc, idx):
    st = LM.Store(1 << 16)
    st.put(sc["keys"][idx], sc["pos"][idx], sc["normal"][idx], sc["min_dist"][idx], sc["max_dist"][idx], sc["pdesc"][idx], sc["flags"][idx])
    return st


def tally(code):
    return {PM.EXITS[c]: int((code == c).sum()) for c in range(len(PM.EXITS)) if (code == c).any()}


# ---- the edge scene: every comparison of the two loops on its edge, with hand-placed features ----
# An identity pose, fx = fy = 256 and cx = cy = 0.5 make u = 256 * x + 0.5 exact for z = 1, so a projection can be put exactly on a
# bound and exactly one ulp outside it (the bounds are chosen inside the image for that: 16 and 360 sit where the float grid of
# the sum is no coarser than that of the product).
EDGE_BOUNDS = (f32(16), f32(360), f32(16), f32(224))
EDGE_CASES = ("inside", "u_min", "u_max", "v_min", "v_max", "u_below", "u_above", "v_below", "v_above", "behind", "z_zero", "nan",
              "bad", "key0", "unknown", "near_on", "near_out", "far_on", "far_out", "level_low", "level_high", "octave0", "octave_top",
              "obs_first", "unobs_second", "unobs_first", "obs_second", "xr_inside", "xr_outside", "found")


def _fit_factor(c, dist, want_equal_then):
    """Floats m around dist / c with c * m == dist, and the neighbour on the `want_equal_then` side (+1: the next m up, whose
    product exceeds dist; -1: the next m down, whose product is below); None when no m gives equality."""
    m = f32(f64(dist) / f64(c))
    for _ in range(8):
        m = np.nextafter(m, f32(0))
    for _ in range(17):
        if f32(c * m) == dist:
            o = m
            while f32(c * o) == dist:
                o = np.nextafter(o, f32(np.inf) if want_equal_then > 0 else f32(0))
            return m, o
        m = np.nextafter(m, f32(np.inf))
    return None


def edge_scene(oracle=None):
    from orbhip import capi, guided
    rng = np.random.default_rng(101)
    nc = len(EDGE_CASES)
    ix = {c: i for i, c in enumerate(EDGE_CASES)}
    sf = (LS.S ** np.arange(LS.NLEVELS)).astype(f32)
    cam = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), Ow=np.zeros(3, f32), fx=f32(256), fy=f32(256), cx=f32(0.5), cy=f32(0.5),
               mbf=f32(32), bounds=EDGE_BOUNDS, scale_factors=sf, log_scale_factor=f32(np.log(LS.S)), viewing_cos_limit=f32(0.5))
    # where each case projects: on a lattice unless the case says otherwise
    uv = np.array([[40 + 24 * (k % 12), 40 + 30 * (k // 12)] for k in range(nc)], f32)
    up, dn = f32(np.inf), f32(-np.inf)
    uv[ix["u_min"]], uv[ix["u_max"]] = (16, 100), (360, 100)
    uv[ix["v_min"]], uv[ix["v_max"]] = (100, 16), (100, 224)
    uv[ix["u_below"]], uv[ix["u_above"]] = (np.nextafter(f32(16), dn), 130), (np.nextafter(f32(360), up), 130)
    uv[ix["v_below"]], uv[ix["v_above"]] = (130, np.nextafter(f32(16), dn)), (130, np.nextafter(f32(224), up))
    uv[ix["unobs_second"]] = uv[ix["obs_first"]]
    uv[ix["obs_second"]] = uv[ix["unobs_first"]]
    pos = np.zeros((nc, 3), f32)
    pos[:, :2] = ((uv.astype(f64) - 0.5) / 256).astype(f32)
    pos[:, 2] = 1
    assert np.array_equal(pos[:, :2].astype(f64) * 256 + 0.5, uv.astype(f64))     # exact, so the device has no freedom either
    pos[ix["behind"]] = -pos[ix["behind"]]
    pos[ix["z_zero"], 2] = 0
    pos[ix["nan"], 1] = np.nan
    with np.errstate(all="ignore"):
        dist = np.sqrt((pos.astype(f64) ** 2).sum(axis=1)).astype(f32)
    mn, mx = (dist / f32(2)).astype(f32), (dist * f32(2)).astype(f32)
    mn[~np.isfinite(dist)], mx[~np.isfinite(dist)] = 0.5, 2
    for on, out, c, side in (("near_on", "near_out", f32(0.8), +1), ("far_on", "far_out", f32(1.2), -1)):
        # move the pair along the lattice row until c * m == dist has a solution
        for shift in range(64):
            for k in (ix[on], ix[out]):
                pos[k, 0] = f32((f64(uv[k, 0]) + shift * 0.25 - 0.5) / 256)
            d = f32(np.sqrt((pos[ix[on]].astype(f64) ** 2).sum()))
            fit = _fit_factor(c, d, side)
            if fit is not None and np.array_equal(pos[ix[on]], pos[ix[on]]):
                break
        assert fit is not None
        pos[ix[out]] = pos[ix[on]]
        dist[ix[on]] = dist[ix[out]] = d
        if side > 0:
            mn[ix[on]], mn[ix[out]] = fit
            mx[ix[on]] = mx[ix[out]] = d * f32(2)
        else:
            mx[ix[on]], mx[ix[out]] = fit
            mn[ix[on]] = mn[ix[out]] = d / f32(4)
    mx[ix["level_low"]], mn[ix["level_low"]] = dist[ix["level_low"]] / f32(1.15), dist[ix["level_low"]] / f32(4.6)
    mx[ix["level_high"]], mn[ix["level_high"]] = dist[ix["level_high"]] * f32(1.2 ** 9.5), dist[ix["level_high"]] / f32(1.1)
    # the current frame: one feature per case where the case projects (clamped into the image), descriptors of its own
    n = nc
    kps = np.zeros(n, capi.KP_DTYPE)
    with np.errstate(all="ignore"):
        pu = (f32(256) * pos[:, 0] / pos[:, 2] + f32(0.5)).astype(f32)
        pv = (f32(256) * pos[:, 1] / pos[:, 2] + f32(0.5)).astype(f32)
    kps["x"] = np.where(np.isfinite(pu), np.clip(pu, 1, W - 1), 50)
    kps["y"] = np.where(np.isfinite(pv), np.clip(pv, 1, H - 1), 50)
    kps["size"], kps["angle"], kps["response"], kps["octave"], kps["class_id"] = 31, 10, 50, 3, -1
    kps["octave"][ix["octave0"]], kps["octave"][ix["octave_top"]] = 1, LS.NLEVELS - 1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pdesc = desc.copy()
    for j in range(nc):
        for b in rng.integers(0, 256, 6):
            pdesc[j, b >> 3] ^= np.uint8(1 << (b & 7))
    pdesc[ix["unobs_second"]] = pdesc[ix["obs_first"]]
    pdesc[ix["obs_second"]] = pdesc[ix["unobs_first"]]
    src_kps = np.zeros(nc, capi.KP_DTYPE)
    src_kps["size"], src_kps["angle"], src_kps["octave"], src_kps["class_id"] = 31, 10, 2, -1
    src_kps["octave"][ix["octave0"]], src_kps["octave"][ix["octave_top"]] = 0, LS.NLEVELS - 1
    src_kps["x"], src_kps["y"] = kps["x"], kps["y"]
    flags = np.ones(nc, np.uint8)
    flags[ix["bad"]] |= 2
    flags[ix["unobs_second"]] = flags[ix["unobs_first"]] = 0
    keys = (np.arange(nc, dtype=np.uint64) + np.uint64(1)) * np.uint64(104729)
    hold = keys.copy()
    hold[ix["key0"]] = 0
    unknown = np.zeros(nc, bool)
    unknown[ix["unknown"]] = True
    u_right = np.full(n, -1, f32)
    sc = dict(name="edge", th=f32(7), th_high=100, kps=kps, desc=desc, gp=guided.grid_params(0, W, 0, H), cam=cam, src_kps=src_kps,
              src_desc=pdesc, keys=keys, pos=pos, normal=np.tile(np.array([0, 0, 1], f32), (nc, 1)), min_dist=mn, max_dist=mx,
              pdesc=pdesc, flags=flags, hold=hold, unknown=unknown, found=keys[[ix["found"]]], occupied=np.zeros(n, np.uint8),
              u_right=u_right, ix=ix)
    # the right coordinate of two features: |proj_xr - u_right| equal to the radius (inside) and one float beyond (outside)
    st = model_store(sc, stored(sc, True))
    q, code, _ = PM.last_frame_queries(st, cam, sc["th"], hold, src_kps, PM.SAME)
    for case, outside in (("xr_inside", False), ("xr_outside", True)):
        k = ix[case]
        assert code[k] == PM.ACTIVE
        ur = f32(q["proj_xr"][k] + q["radius"][k])
        while abs(f32(q["proj_xr"][k] - ur)) > q["radius"][k]:
            ur = np.nextafter(ur, dn)
        while abs(f32(q["proj_xr"][k] - np.nextafter(ur, up))) <= q["radius"][k]:
            ur = np.nextafter(ur, up)
        u_right[k] = np.nextafter(ur, up) if outside else ur
        assert u_right[k] > 0
    return sc


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    for name in SCENES:
        sc = make(oracle, name)
        st = model_store(sc, stored(sc, True))
        for mo in ((0,) if name == "mono" else (0, 1, 2)):
            q, code, qd, na, nm, match = PM.search_last_frame(oracle, st, sc["cam"], sc["th"], sc["hold"], sc["src_kps"], mo, sc["kps"],
                                                              sc["desc"], sc["gp"], sc["u_right"], sc["occupied"], True, sc["th_high"])
            print(name, "last", mo, len(sc["kps"]), len(sc["hold"]), "active", na, "matches", nm, "-2:", int((match == -2).sum()),
                  "twice", PM.claimed_twice(oracle, q, qd, sc["kps"], sc["desc"], sc["gp"], sc["u_right"], sc["occupied"]), tally(code))
        st = model_store(sc, stored(sc, False))
        q, code, qd, na, nm, match = PM.search_keyframe_points(oracle, st, sc["cam"], sc["th"], row_keys(sc), sc["found"], sc["src_kps"],
                                                               sc["kps"], sc["desc"], sc["gp"], sc["occupied"], True, sc["th_high"])
        print(name, "kf", "active", na, "matches", nm, "-2:", int((match == -2).sum()),
              "twice", PM.claimed_twice(oracle, q, qd, sc["kps"], sc["desc"], sc["gp"], None, sc["occupied"]), tally(code))
