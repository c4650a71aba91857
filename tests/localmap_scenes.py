"""Scenes of the local-map tests: a frame of the synthetic stream, a camera with a small motion against its neighbour, and map
points made by back-projecting the neighbouring frame's key points at random depths, with normals and distance ranges drawn so
that every exit of Frame::isInFrustum and every scale level is taken (tests/test_localmap_gpu.py asserts a floor on each tally;
`python tests/localmap_scenes.py` prints the tallies from the model alone, no device)."""
import struct

import numpy as np

import localmap_model as M

f32, f64 = np.float32, np.float64
SCENES = {"640x480": (640, 480, 0.0, 41), "752x480": (752, 480, 0.0, 43), "1241x376_stereo": (1241, 376, 386.0, 47)}
S = f32(1.2)
NLEVELS = 8
FLOOR = 20


def _rot(axis, ang):
    axis = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def pose(rng, ang=0.002, shift=0.01):
    """(Rcw, tcw, Ow) as float32; Ow = -Rcw' tcw as the caller's Frame::UpdatePoseMatrices would hold it."""
    R = _rot(rng.standard_normal(3), ang).astype(f32)
    t = (rng.standard_normal(3) * shift).astype(f32)
    Ow = (-(R.astype(f64).T @ t.astype(f64))).astype(f32)
    return R, t, Ow


def make(oracle, name, npoints=2600, nfeatures=1000):
    from orbhip import guided, synth
    w, h, mbf, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    frames = synth.make_frames(seed, w, h, 2)
    ref = oracle.Extractor(nfeatures)
    (kA, dA), (kB, dB) = ref(frames[0]), ref(frames[1])
    sf = (S ** np.arange(NLEVELS)).astype(f32)
    R, t, Ow = pose(rng)
    cam = dict(Rcw=R, tcw=t, Ow=Ow, fx=f32(0.8 * w), fy=f32(0.82 * w), cx=f32(w / 2 - 0.5), cy=f32(h / 2 + 0.5), mbf=f32(mbf),
               bounds=(f32(0), f32(w), f32(0), f32(h)), scale_factors=sf, log_scale_factor=f32(np.log(S)), viewing_cos_limit=f32(0.5))
    pts = map_points(rng, cam, kB, dB, npoints, w, h)
    sc = dict(name=name, w=w, h=h, kps=kA, desc=dA, gp=guided.grid_params(0, w, 0, h), cam=cam, **pts)
    n = len(kA)
    sc["occupied"] = (rng.random(n) < 0.1).astype(np.uint8)
    sc["u_right"] = None
    if mbf:
        ur = kA["x"] - f32(mbf) / rng.uniform(2, 30, n).astype(f32)
        sc["u_right"] = np.where(rng.random(n) < 0.7, ur, f32(-1)).astype(f32)
    return sc


def map_points(rng, cam, kB, dB, npoints, w, h):
    R, t = cam["Rcw"].astype(f64), cam["tcw"].astype(f64)
    fx, fy, cx, cy = (f64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    s = f64(S)
    pos, nrm, mn, mx = np.zeros((npoints, 3), f32), np.zeros((npoints, 3), f32), np.zeros(npoints, f32), np.zeros(npoints, f32)
    desc = np.zeros((npoints, 32), np.uint8)
    kinds = rng.choice(9, npoints, p=[0.52] + [0.06] * 8)    # 0 = meant to be in view, 1..8 = meant for that exit
    for j in range(npoints):
        i = j % len(kB)
        x, y, z, kind = f64(kB["x"][i]), f64(kB["y"][i]), rng.uniform(1, 8), kinds[j]
        if kind == M.LEFT:
            x = -rng.uniform(1, 60)
        elif kind == M.RIGHT:
            x = w + rng.uniform(1, 60)
        elif kind == M.TOP:
            y = -rng.uniform(1, 60)
        elif kind == M.BOTTOM:
            y = h + rng.uniform(1, 60)
        Pc = np.array([(x - cx) * z / fx, (y - cy) * z / fy, z])
        if kind == M.BEHIND:
            Pc = -Pc
        Pw = R.T @ (Pc - t)
        d = Pw - cam["Ow"].astype(f64)
        dist = np.linalg.norm(d)
        d /= dist
        e = np.cross(d, rng.standard_normal(3))
        e /= np.linalg.norm(e)
        if kind == M.VIEWCOS:
            a = np.radians(rng.uniform(61, 120))
        else:
            a = np.radians(rng.uniform(0, 3.4) if rng.random() < 0.5 else rng.uniform(3.8, 58))
        n = np.cos(a) * d + np.sin(a) * e
        if rng.random() < 0.5:      # the level of the source key point or the one above: these find their feature
            lv = min(int(kB["octave"][i]) + int(rng.integers(0, 2)), NLEVELS - 1)
        else:                       # every level, and ratios beyond both ends (clamped)
            lv = int(rng.integers(-1, NLEVELS + 1))
        ratio = s ** (lv - rng.uniform(0.1, 0.9))
        hi = ratio * dist
        lo = hi / s ** (NLEVELS - 1)
        if kind == M.NEAR:
            lo = dist * rng.uniform(1.3, 2.0)
            hi = lo * s ** (NLEVELS - 1)
        elif kind == M.FAR:
            hi = dist * rng.uniform(0.3, 0.8)
            lo = hi / s ** (NLEVELS - 1)
        pos[j], nrm[j], mn[j], mx[j] = Pw, n, lo, hi
        desc[j] = dB[i]
        for b in rng.integers(0, 256, int(rng.integers(0, 12))):
            desc[j, b >> 3] ^= np.uint8(1 << (b & 7))
    flags = (rng.random(npoints) < 0.7).astype(np.uint8) | ((rng.random(npoints) < 0.03).astype(np.uint8) << 1)
    keys = (rng.permutation(npoints).astype(np.uint64) + np.uint64(1)) * np.uint64(7919)
    assert np.isfinite(pos).all() and np.isfinite(nrm).all() and (mn > 0).all() and (mx > mn).all()
    return dict(keys=keys, pos=pos, normal=nrm, min_dist=mn, max_dist=mx, pdesc=desc, flags=flags)


def tallies(code, rec):
    exits = {M.EXITS[c]: int((code == c).sum()) for c in range(1, 9)}
    levels = {lv: int(((rec["in_view"] == 1) & (rec["level"] == lv)).sum()) for lv in range(NLEVELS)}
    return exits, levels


def write_scene(path, sc, th, skip, occ_kind):
    """The scene as test_localmap_dropin reads it (struct Head, then the frame, then the points)."""
    cam = sc["cam"]
    n, nq = len(sc["kps"]), len(sc["keys"])
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = cam["Rcw"], cam["tcw"]
    sf = np.zeros(16, f32)
    sf[:len(cam["scale_factors"])] = cam["scale_factors"]
    b = cam["bounds"]
    head = struct.pack("<4i12f", n, nq, len(cam["scale_factors"]), 0 if sc["u_right"] is None else 1, cam["fx"], cam["fy"], cam["cx"],
                       cam["cy"], cam["mbf"], b[0], b[1], b[2], b[3], cam["log_scale_factor"], th, cam["viewing_cos_limit"])
    ur = np.full(n, -1, f32) if sc["u_right"] is None else sc["u_right"].astype(f32)
    rec = np.concatenate([sc["pos"], sc["normal"], sc["min_dist"][:, None], sc["max_dist"][:, None]], axis=1).astype(f32)
    with open(path, "wb") as f:
        f.write(head + T.tobytes() + sf.tobytes() + np.ascontiguousarray(sc["kps"]).tobytes() + np.ascontiguousarray(sc["desc"]).tobytes() +
                ur.tobytes() + occ_kind.astype(np.uint8).tobytes() + rec.tobytes() + np.ascontiguousarray(sc["pdesc"]).tobytes() +
                sc["flags"].astype(np.uint8).tobytes() + skip.astype(np.uint8).tobytes())


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    for name in SCENES:
        sc = make(oracle, name)
        rec, code = M.frustum(sc["cam"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
        d = np.linalg.norm(sc["pos"].astype(f64) - sc["cam"]["Ow"].astype(f64), axis=1)
        print(name, len(sc["kps"]), "features; dist > 0:", bool((d > 0).all()), tallies(code, rec))
