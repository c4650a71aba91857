"""Scenes of the Fuse tests (tests/test_fuse_model.py on the CPU, tests/test_fuse_gpu.py on the device).

make():        a 376 x 241 frame of the synthetic stream is target key frame 0; the source key frame's points are made by
               back-projecting the target's own key points through its camera (tests/localmap_scenes.map_points, so every exit of
               the projection loop is taken), displaced by a pixel or two so that both chi-square gates decide both ways.  Five
               target records over four resident sets of different sizes (one key twice, with another th), stereo and monocular.
edge_scene():  every comparison of the loop on its edge, hand-placed (identity pose, fx = fy = 256, cx = cy = 0.5 and z = 1 make
               u = 256 * x + 0.5 exact, so a projection can sit exactly on a bound and one ulp either side of it).
assoc_scene(): a point for which fx * (xc * invz) + cx and (fx * xc) * invz + cx differ, with the target's mnMaxX put between them.
`python tests/fuse_scenes.py` prints the tallies from the model alone, no device."""
import numpy as np

import fuse_model as FM
import localmap_scenes as LS
from projtrack_scenes import _fit_factor

f32, f64 = np.float32, np.float64
W, H = 376, 241
SRC_ROW, CUR_ROW = 0x700, 0x701          # key-frame rows: the source of the first pass, the target's own of the second
SET_A, SET_B, SET_C, SET_D = 0x710, 0x711, 0x712, 0x713
SIZES = (1, 63, 64, 65, 255, 256, 257)


def scale_tables():
    sf = (LS.S ** np.arange(LS.NLEVELS)).astype(f32)
    sig = (f32(1.0) / (sf * sf)).astype(f32)          # KeyFrame::mvInvLevelSigma2
    return sf, sig


def _camera(R, t, Ow, mbf, bounds=None):
    sf, _ = scale_tables()
    return dict(Rcw=R, tcw=t, Ow=Ow, fx=f32(0.8 * W), fy=f32(0.82 * W), cx=f32(W / 2 - 0.5), cy=f32(H / 2 + 0.5), mbf=f32(mbf),
                bounds=bounds or (f32(0), f32(W), f32(0), f32(H)), scale_factors=sf, log_scale_factor=f32(np.log(LS.S)),
                viewing_cos_limit=f32(0.5))


def _nudged(rng, cam, ang=0.0004, shift=0.002):
    """The camera a little way off: projections move by a fraction of a pixel to a few pixels."""
    dR, dt, _ = LS.pose(rng, ang, shift)
    R = (dR.astype(f64) @ cam["Rcw"].astype(f64)).astype(f32)
    t = (dR.astype(f64) @ cam["tcw"].astype(f64) + dt.astype(f64)).astype(f32)
    Ow = (-(R.astype(f64).T @ t.astype(f64))).astype(f32)
    return dict(cam, Rcw=R, tcw=t, Ow=Ow)


def make(oracle, seed=11, nfeatures=500, npoints=420):
    from orbhip import guided, synth
    rng = np.random.default_rng(seed)
    frames = synth.make_frames(seed, W, H, 2)
    ref = oracle.Extractor(nfeatures)
    (kA, dA), (kB, dB) = ref(frames[0]), ref(frames[1])
    sf, sig = scale_tables()
    R, t, Ow = LS.pose(rng)
    cam0 = _camera(R, t, Ow, 40.0)
    npoints = min(npoints, len(kA))
    pts = LS.map_points(rng, cam0, kA, dA, npoints, W, H)
    # displace every point sideways in the camera frame by (dx, dy) pixels at its depth: the reprojection error the gates test
    Pc = (cam0["Rcw"].astype(f64) @ pts["pos"].astype(f64).T).T + cam0["tcw"].astype(f64)
    z = Pc[:, 2]
    px = rng.normal(0, 1.3, (npoints, 2)) * sf[np.clip(kA["octave"][:npoints], 0, LS.NLEVELS - 1)][:, None]
    d_cam = np.stack([px[:, 0] * z / f64(cam0["fx"]), px[:, 1] * z / f64(cam0["fy"]), np.zeros(npoints)], axis=1)
    pts["pos"] = (pts["pos"].astype(f64) + d_cam @ cam0["Rcw"].astype(f64)).astype(f32)
    # the right coordinates of set A agree with the depth of the point on each feature, to a pixel or so
    n = len(kA)
    urA = kA["x"] - f32(40.0) / rng.uniform(1, 8, n).astype(f32)
    with np.errstate(all="ignore"):
        urA[:npoints] = np.where(z > 0.5, kA["x"][:npoints] - 40.0 / np.abs(z) + rng.normal(0, 1.0, npoints) * sf[kA["octave"][:npoints]],
                                 urA[:npoints])
    urA = np.where(rng.random(n) < 0.7, urA, -1).astype(f32)
    gp = guided.grid_params(0, W, 0, H)
    nB = int(0.6 * n)
    sets = {SET_A: (kA, dA), SET_B: (kA[:nB].copy(), dA[:nB].copy()), SET_C: (kB, dB), SET_D: (kA[::2].copy(), dA[::2].copy())}
    cams = [cam0, _nudged(rng, cam0), _nudged(rng, cam0, 0.001, 0.004), cam0, dict(_nudged(rng, cam0), mbf=f32(25.0))]
    ths = [f32(3.0), f32(3.0), f32(5.0), f32(6.0), f32(3.0)]
    urs = [urA, None, None, urA, urA[::2].copy()]
    targets = [dict(key=k, cam=c, th=th, kps=sets[k][0], desc=sets[k][1], gp=gp, u_right=ur, sig=sig)
               for k, c, th, ur in zip((SET_A, SET_B, SET_C, SET_A, SET_D), cams, ths, urs)]
    row = pts["keys"].copy()
    r = rng.random(npoints)
    row[r < 0.06] = 0
    stale = np.nonzero((r >= 0.06) & (r < 0.10))[0]      # put, entered in the row, then erased from the store
    skip = (rng.random((len(targets), npoints)) < 0.1).astype(np.uint8)
    return dict(targets=targets, sets=sets, row=row, skip=skip, stale=stale, **pts)


def model_store(sc, without_stale=True):
    st = FM.Store(1 << 16)
    st.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
    if without_stale:
        st.erase(sc["keys"][sc["stale"]])
    return st


# ---- the edge scene ----
EDGE_BOUNDS = (f32(16), f32(360), f32(16), f32(224))
EDGE_CASES = ("inside", "u_min", "u_min_below", "u_min_above", "u_max", "u_max_below", "u_max_above", "v_min", "v_min_below",
              "v_min_above", "v_max", "v_max_below", "v_max_above", "behind", "z_zero", "nan", "bad", "key0", "stale", "skipped",
              "near_on", "near_out", "far_on", "far_out", "view_on", "view_out", "level_low", "level_high", "gate_mono_on",
              "gate_mono_out", "gate_stereo_on", "gate_stereo_out")
# what the model must say of each case (tests/test_fuse_model.py); None: only "not active"
EDGE_EXPECT = dict(inside=FM.ACTIVE, u_min=FM.ACTIVE, u_min_below=FM.LEFT, u_min_above=FM.ACTIVE, u_max=FM.RIGHT, u_max_below=FM.ACTIVE,
                   u_max_above=FM.RIGHT, v_min=FM.ACTIVE, v_min_below=FM.TOP, v_min_above=FM.ACTIVE, v_max=FM.BOTTOM,
                   v_max_below=FM.ACTIVE, v_max_above=FM.BOTTOM, behind=FM.BEHIND, z_zero=None, nan=FM.NONFINITE, bad=FM.BAD,
                   key0=FM.NO_POINT, stale=FM.UNKNOWN, skipped=FM.SKIPPED, near_on=FM.ACTIVE, near_out=FM.NEAR, far_on=FM.ACTIVE,
                   far_out=FM.FAR, view_on=FM.ACTIVE, view_out=FM.VIEW, level_low=FM.ACTIVE, level_high=FM.ACTIVE,
                   gate_mono_on=FM.ACTIVE, gate_mono_out=FM.ACTIVE, gate_stereo_on=FM.ACTIVE, gate_stereo_out=FM.ACTIVE)
GATE_LEVELS = dict(gate_mono_on=1, gate_mono_out=2, gate_stereo_on=5, gate_stereo_out=6)


def gate_limits(lim):
    """(the largest float not above lim, the float after it): a float product is never equal to 5.99 or 7.8."""
    a = f32(lim)
    if float(a) > lim:
        a = np.nextafter(a, f32(-np.inf))
    return a, np.nextafter(a, f32(np.inf))


def edge_scene():
    from orbhip import capi, guided
    rng = np.random.default_rng(103)
    nc = len(EDGE_CASES)
    ix = {c: i for i, c in enumerate(EDGE_CASES)}
    sf, sig = scale_tables()
    sig = sig.copy()
    cam = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), Ow=np.zeros(3, f32), fx=f32(256), fy=f32(256), cx=f32(0.5), cy=f32(0.5),
               mbf=f32(32), bounds=EDGE_BOUNDS, scale_factors=sf, log_scale_factor=f32(np.log(LS.S)), viewing_cos_limit=f32(0.5))
    uv = np.array([[40 + 24 * (k % 12), 40 + 30 * (k // 12)] for k in range(nc)], f32)
    up, dn = f32(np.inf), f32(-np.inf)
    for a, (lo, hi), col in (("u", EDGE_BOUNDS[:2], 0), ("v", EDGE_BOUNDS[2:], 1)):
        for case, val, other in ((a + "_min", lo, 100), (a + "_min_below", np.nextafter(lo, dn), 130), (a + "_min_above", np.nextafter(lo, up), 160),
                                 (a + "_max", hi, 100), (a + "_max_below", np.nextafter(hi, dn), 130), (a + "_max_above", np.nextafter(hi, up), 160)):
            uv[ix[case], col], uv[ix[case], 1 - col] = val, other
    pos = np.zeros((nc, 3), f32)
    pos[:, :2] = ((uv.astype(f64) - 0.5) / 256).astype(f32)
    pos[:, 2] = 1
    assert np.array_equal(pos[:, :2].astype(f64) * 256 + 0.5, uv.astype(f64))     # exact, so the device has no freedom either

    def norm(p):
        return f32(np.sqrt((p.astype(f64) ** 2).sum()))

    mn, mx = np.zeros(nc, f32), np.zeros(nc, f32)
    for on, out, c, side in (("near_on", "near_out", f32(0.8), +1), ("far_on", "far_out", f32(1.2), -1)):
        fit = None
        for shift in range(64):          # along the lattice row until c * m == dist has a solution
            for k in (ix[on], ix[out]):
                pos[k, 0] = f32((f64(uv[ix[on], 0]) + shift * 0.25 - 0.5) / 256)
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
    normal = np.tile(np.array([0, 0, 1], f32), (nc, 1))
    normal[ix["view_on"], 2] = f32(0.5) * dist[ix["view_on"]]             # PO . n = 1 * nz: exactly 0.5 * dist3D
    normal[ix["view_out"], 2] = np.nextafter(f32(0.5) * dist[ix["view_out"]], dn)
    mx[ix["level_low"]], mn[ix["level_low"]] = dist[ix["level_low"]] / f32(1.15), dist[ix["level_low"]] / f32(4.6)
    mx[ix["level_high"]], mn[ix["level_high"]] = dist[ix["level_high"]] * f32(1.2 ** 9.5), dist[ix["level_high"]] / f32(1.1)
    for case, lv in GATE_LEVELS.items():
        mx[ix[case]] = dist[ix[case]] * f32(1.2 ** (lv - 0.5))
    pos[ix["behind"]] = -pos[ix["behind"]]
    pos[ix["z_zero"], 2] = 0
    pos[ix["nan"], 1] = np.nan
    # the target's features: one where each case projects (clamped into the image), octave 3: inside [level - 1, level] of ratio 2
    kps = np.zeros(nc, capi.KP_DTYPE)
    kps["x"], kps["y"] = np.clip(uv[:, 0], 1, W - 1), np.clip(uv[:, 1], 1, H - 1)
    kps["size"], kps["angle"], kps["response"], kps["octave"], kps["class_id"] = 31, 10, 50, 3, -1
    kps["octave"][ix["level_low"]], kps["octave"][ix["level_high"]] = 0, LS.NLEVELS - 1
    kps["octave"][ix["far_on"]] = kps["octave"][ix["far_out"]] = 0
    u_right = np.full(nc, -1, f32)
    a599, b599 = gate_limits(5.99)
    a78, b78 = gate_limits(7.8)
    for case, lim in (("gate_mono_on", a599), ("gate_mono_out", b599), ("gate_stereo_on", a78), ("gate_stereo_out", b78)):
        k, lv = ix[case], GATE_LEVELS[case]
        kps["x"][k] = uv[k, 0] - 2                                        # ex = 2, ey = 0 (er = 0): e2 = 4
        kps["octave"][k] = lv
        sig[lv] = lim / f32(4)                                            # so that e2 * sigma = lim exactly
        if "stereo" in case:
            u_right[k] = uv[k, 0] - f32(32)                               # = proj_xr: u - mbf * invz with invz = 1
    desc = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    pdesc = desc.copy()
    for j in range(nc):
        for b in rng.integers(0, 256, 6):
            pdesc[j, b >> 3] ^= np.uint8(1 << (b & 7))
    flags = np.ones(nc, np.uint8)
    flags[ix["bad"]] |= 2
    keys = (np.arange(nc, dtype=np.uint64) + np.uint64(1)) * np.uint64(104723)
    row = keys.copy()
    row[ix["key0"]] = 0
    skip = np.zeros((1, nc), np.uint8)
    skip[0, ix["skipped"]] = 1
    target = dict(key=SET_A, cam=cam, th=f32(3.0), kps=kps, desc=desc, gp=guided.grid_params(0, W, 0, H), u_right=u_right, sig=sig)
    return dict(targets=[target], sets={SET_A: (kps, desc)}, row=row, skip=skip, stale=np.array([ix["stale"]]), keys=keys, pos=pos,
                normal=normal, min_dist=mn, max_dist=mx, pdesc=pdesc, flags=flags, ix=ix)


def assoc_scene():
    """One point whose u differs between the two associations; the target's mnMaxX is the larger of the two values, so exactly one
    of them is inside (u < max_x).  Returns (scene, u of Fuse, u of the frame searches)."""
    from orbhip import capi, guided
    rng = np.random.default_rng(7)
    sf, sig = scale_tables()
    R, t, Ow = LS.pose(rng)
    cam = _camera(R, t, Ow, 40.0)
    while True:
        Pc = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(1, 8)])
        Pw = (cam["Rcw"].astype(f64).T @ (Pc - cam["tcw"].astype(f64))).astype(f32)
        ua = FM.project(cam, Pw)[2][0]
        ub = FM.project(cam, Pw, other_association=True)[2][0]
        if ua != ub and 20 < ua < W - 20:
            break
    cam = dict(cam, bounds=(f32(0), max(ua, ub), f32(0), f32(H)))
    d = f32(np.linalg.norm(Pw.astype(f64) - cam["Ow"].astype(f64)))
    nrm = ((Pw.astype(f64) - cam["Ow"].astype(f64)) / f64(d)).astype(f32)
    v = FM.project(cam, Pw)[3][0]
    kps = np.zeros(1, capi.KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["octave"], kps["class_id"] = min(ua, ub), v, 31, 3, -1
    desc = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    keys = np.array([424243], np.uint64)
    target = dict(key=SET_A, cam=cam, th=f32(3.0), kps=kps, desc=desc, gp=guided.grid_params(0, W, 0, H), u_right=None, sig=sig)
    sc = dict(targets=[target], sets={SET_A: (kps, desc)}, row=keys.copy(), skip=np.zeros((1, 1), np.uint8), stale=np.zeros(0, np.int64),
              keys=keys, pos=Pw.reshape(1, 3), normal=nrm.reshape(1, 3), min_dist=np.array([d / f32(2)], f32),
              max_dist=np.array([d * f32(2)], f32), pdesc=desc.copy(), flags=np.ones(1, np.uint8))
    return sc, ua, ub


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    for name, sc in (("main", make(oracle)), ("edge", edge_scene())):
        st = model_store(sc)
        for k, T in enumerate(sc["targets"]):
            stats = {}
            q, code, qd, na, bi, bd = FM.fuse(oracle, st, T, T["th"], sc["row"], sc["skip"][k], stats)
            print(name, k, len(T["kps"]), "features", len(sc["row"]), "entries; active", na, "fused", int((bd <= FM.TH_LOW).sum()), stats,
                  FM.tally(code))
    sc, ua, ub = assoc_scene()
    print("assoc", repr(ua), repr(ub), sc["targets"][0]["cam"]["bounds"][1])
