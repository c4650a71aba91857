"""Edge scenes of the local-map tests: inputs that sit exactly on every comparison k_local_frustum decides on, and one float step
(np.nextafter) to each side.  Plain numpy plus the independent model (tests/localmap_model.py), no device.  It starts from the
points of a tests/localmap_scenes.py scene that the model reports in view and derives, per edge kind, cases of the form
(kind, side, camera, point, the exit code or level meant for it); verify() evaluates every case with the model alone and asserts
that it got what was meant and a floor on each tally (`python tests/localmap_edges.py` prints the tallies).

Cameras: "base" (the scene's own, shared by the near / far / level / 0.998 cases), three degenerate ones for the sign of PcZ
("pcz_sum", "pcz_raw", "pcz_neg"), and ROWS numbered rows for the batched device form -- the edges that are camera parameters
(image bounds, viewing_cos_limit, th, the pyramid shape).  Consecutive rows alternate (log_scale_factor, nlevels)."""
import numpy as np

import localmap_model as M
import localmap_scenes as scenes

f32, f64 = np.float32, np.float64
# the issue's shapes plus (1.08, 8): two shapes with equal nlevels and different scale factors, for the table cache.  In this
# order every neighbouring pair differs, (1.2, 8) | (1.08, 8) share nlevels and (1.2, 1) | (1.2, 2) share the scale factor.
SHAPES = ((1.2, 8), (1.08, 8), (1.08, 16), (1.2, 1), (1.2, 2), (2.0, 5), (1.5, 12))
BASE_SHAPE = (1.2, 8)
FLOOR, FLOOR_SMALL = 20, 4
TH3 = (f32(1.0), np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0)))
NBOUND_ROWS = 60            # 20 rows per side: each row carries one case of each of the four bounds and of the limit
SIDES = ("at", "inside", "outside")
BOUNDS = ("min_x", "max_x", "min_y", "max_y")
PLANT = 3.25                # a planted feature lies at 3.25 * scale factor from the projection: inside radius 4.0, outside 2.5


def up(x, n=1):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf) if n > 0 else f32(-np.inf))
    return x


def shape_params(shape):
    s, nl = shape
    return (f32(s) ** np.arange(nl)).astype(f32), f32(np.log(f32(s)))


def dist_of(cam, pos):
    """|P - Ow| as the model rounds it (float difference, double sum, one rounding)."""
    PO = np.asarray(pos, f32).reshape(-1, 3) - np.asarray(cam["Ow"], f32).reshape(1, 3)
    return np.sqrt((PO.astype(f64) ** 2) @ np.ones(3)).astype(f32), PO


def _dist1(cam, p):
    PO = np.asarray(p, f32) - np.asarray(cam["Ow"], f32)
    sq = f64(0)
    for k in range(3):
        sq = sq + f64(PO[k]) * f64(PO[k])
    return f32(np.sqrt(sq)), PO


def _around(x, n=3):
    return [up(x, k) for k in range(-n, n + 1)]


class _Scene:
    """The growing point list and the cases."""

    def __init__(self, sc):
        self.sc = sc
        self.pos, self.nrm = list(sc["pos"]), list(sc["normal"])
        self.mn, self.mx = list(sc["min_dist"]), list(sc["max_dist"])
        self.desc = list(sc["pdesc"])
        self.cases = []          # (kind, side, camera id, point index, wanted exit code, wanted level or None)
        self.planted = {}        # point index -> (feature index, offset in pixels at scale factor 1)

    def add(self, src, normal=None, mn=None, mx=None, desc=None, pos=None):
        self.pos.append(np.array(self.pos[src] if pos is None else pos, f32))
        self.nrm.append(np.array(self.nrm[src] if normal is None else normal, f32))
        self.mn.append(f32(self.mn[src] if mn is None else mn))
        self.mx.append(f32(self.mx[src] if mx is None else mx))
        self.desc.append(np.array(self.desc[src] if desc is None else desc, np.uint8))
        return len(self.pos) - 1

    def case(self, kind, side, cam_id, idx, code, level=None):
        self.cases.append((kind, side, cam_id, idx, code, level))


def _near_far(E, cam, cand, rng):
    """f32(0.8) * min_dist == dist and f32(1.2) * max_dist == dist exactly, and the neighbours that fall on each side."""
    found = {"near": 0, "far": 0}
    tried = {"near": 0, "far": 0}
    for kind, c, code_out in (("near", f32(0.8), M.NEAR), ("far", f32(1.2), M.FAR)):
        for i in cand:
            if found[kind] >= FLOOR:
                break
            tried[kind] += 1
            d = _dist1(cam, E.pos[i])[0]
            vals = _around(d / c, 6)
            hit = [m for m in vals if c * m == d]
            lo = [m for m in vals if c * m < d]
            hi = [m for m in vals if c * m > d]
            if not hit or not lo or not hi or hit[0] not in _around(d / c, 3):
                continue
            # near: dist < 0.8 min rejects -> the larger min_dist is outside; far: dist > 1.2 max rejects -> the smaller one
            sides = {"at": hit[0], "inside": max(lo) if kind == "near" else min(hi), "outside": min(hi) if kind == "near" else max(lo)}
            for side, m in sides.items():
                j = E.add(i, mn=m) if kind == "near" else E.add(i, mx=m, mn=m / f32(8))
                E.case(kind, side, "base", j, code_out if side == "outside" else M.IN_VIEW)
            found[kind] += 1
    return tried


def _levels(E, cam, shape, T, cand, per_k):
    """max_dist / dist == T[k] exactly (level k + 1) and the largest max_dist whose ratio is below T[k] (level k), for every k."""
    nl = shape[1]
    it = iter(cand)
    tried = hits = 0
    for k in range(nl - 1):
        got = 0
        while got < per_k:
            i = next(it)
            tried += 1
            d = _dist1(cam, E.pos[i])[0]
            vals = _around(T[k] * d, 6)
            hit = [m for m in vals if m / d == T[k]]
            lo = [m for m in vals if m / d < T[k]]
            if not hit or not lo or hit[0] not in _around(T[k] * d, 3):
                continue
            hits += 1
            got += 1
            E.case("level", "at", shape, E.add(i, mx=hit[0], mn=d / f32(4)), M.IN_VIEW, k + 1)
            E.case("level", "below", shape, E.add(i, mx=max(lo), mn=d / f32(4)), M.IN_VIEW, k)
    # ratios beyond both ends of the table: 0.9 is in the distance range (dist <= 1.2 * 0.9 dist) and below T[0] > 1
    for _ in range(2):
        i = next(it)
        d = _dist1(cam, E.pos[i])[0]
        E.case("clamp", "low", shape, E.add(i, mx=f32(0.9) * d, mn=d / f32(4)), M.IN_VIEW, 0)
        E.case("clamp", "high", shape, E.add(i, mx=f32(100.0 * shape[0] ** nl) * d, mn=d / f32(4)), M.IN_VIEW, nl - 1)
    return tried, hits


def _view_cos_998(E, cam, cand, rng, w, h, sf):
    """Normal s * (unit direction camera -> point): s stepped until the model's view_cos is f32(0.998) exactly, one ulp below
    and one above.  Each case has a descriptor of its own and a planted frame feature at PLANT * scale factor."""
    target = f32(0.998)
    want = {"at": target, "below": up(target, -1), "above": up(target, 1)}
    svals = (np.array([0.99799], f32).view(np.uint32) + np.arange(4000, dtype=np.uint32)).view(f32)    # 4000 one-ulp steps
    found = tried = 0
    dirs = ((1, 0), (-1, 0), (0, 1))
    for i in cand:
        if found >= FLOOR:
            break
        rec, code = M.frustum(cam, [E.pos[i]], [E.nrm[i]], [E.mn[i]], [E.mx[i]])
        margin = 4.5 * float(sf[rec["level"][0]]) + 2
        if not (margin < rec["u"][0] < w - margin and margin < rec["v"][0] < h - margin):
            continue
        tried += 1
        d, PO = _dist1(cam, E.pos[i])
        dhat = (PO.astype(f64) / f64(d)).astype(f32)
        nrm = svals[:, None] * dhat[None, :]                                   # float products, as stored
        dot = np.zeros(len(svals), f64)
        for k in range(3):
            dot = dot + f64(PO[k]) * nrm[:, k].astype(f64)
        vc = (dot / f64(d)).astype(f32)
        pick = {side: np.nonzero(vc == t)[0] for side, t in want.items()}
        if any(len(p) == 0 for p in pick.values()):
            continue
        for (side, p), dxy in zip(pick.items(), dirs):
            j = E.add(i, normal=nrm[p[0]], desc=rng.integers(0, 256, 32).astype(np.uint8))
            E.case("0.998", side, "base", j, M.IN_VIEW, int(rec["level"][0]))
            E.planted[j] = (float(rec["u"][0]), float(rec["v"][0]), dxy, int(rec["level"][0]))
        found += 1
    return tried, found


def _pcz(E, src):
    """PcZ of +0.0f, -0.0f and the smallest normals of either sign.  Three cameras, none of them a pose a tracker would hold (Ow
    is an input of its own, so the point keeps a distance of 2 from it):
      pcz_sum  identity Rcw, tcw = (0, 0, 2), P.z = -2: the double sum -2 + 2 is +0.0;
      pcz_raw  identity Rcw, tcw = 0: PcZ = P.z, so +0.0f and the smallest normals are given directly;
      pcz_neg  Rcw = [[0,0,0],[0,0,0],[1e-30,0,1]]: with an identity Rcw the sum x + (-x) is +0.0 in round-to-nearest and -0.0f
               cannot arise; here the double sum is -1e-60, which rounds to -0.0f, while PcX = PcY = 0."""
    tiny = np.finfo(f32).tiny
    nz = (0, 0, 1)
    cams = {}
    base = dict(E.sc["cam"])
    I = np.eye(3, dtype=f32)
    cams["pcz_sum"] = dict(base, Rcw=I, tcw=np.array([0, 0, 2], f32), Ow=np.array([0, 0, -4], f32))
    cams["pcz_raw"] = dict(base, Rcw=I, tcw=np.zeros(3, f32), Ow=np.array([0, 0, -2], f32))
    Rn = np.zeros((3, 3), f32)
    Rn[2, 0], Rn[2, 2] = f32(1e-30), 1
    cams["pcz_neg"] = dict(base, Rcw=Rn, tcw=np.zeros(3, f32), Ow=np.array([0, 0, -2], f32))

    def pt(cam_id, side, P, code):
        E.case("pcz", side, cam_id, E.add(src, pos=P, normal=nz, mn=1.0, mx=4.0), code, None if code else 4)
    pt("pcz_sum", "+0 PcX=0", (0, 0, -2), M.IN_VIEW)            # u = v = NaN: passes both bound tests
    pt("pcz_sum", "+0 PcX>0", (0.5, 0, -2), M.RIGHT)            # u = +inf
    pt("pcz_sum", "+0 PcX<0", (-0.5, 0, -2), M.LEFT)
    pt("pcz_sum", "+0 PcY>0", (0, 0.5, -2), M.BOTTOM)           # u = NaN passes, v = +inf
    pt("pcz_raw", "+0 PcX=0", (0, 0, 0), M.IN_VIEW)
    pt("pcz_raw", "+tiny PcX=0", (0, 0, tiny), M.IN_VIEW)       # u = cx, v = cy; proj_xr = cx - mbf / tiny = -inf
    pt("pcz_raw", "+tiny PcX>0", (0.5, 0, tiny), M.RIGHT)
    pt("pcz_raw", "-tiny PcX=0", (0, 0, -tiny), M.BEHIND)
    pt("pcz_raw", "-tiny PcX>0", (0.5, 0, -tiny), M.BEHIND)
    pt("pcz_neg", "-0 PcX=0", (-1e-30, 0, 0), M.IN_VIEW)        # -0.0f < 0 is false: invz = -inf, u = v = NaN
    pt("pcz_neg", "+0 PcX=0", (1e-30, 0, 0), M.IN_VIEW)
    return cams


def _rows(E, cam, inview, rec0, rng, shapes):
    """The cameras of the batched form.  Rows 0 .. NBOUND_ROWS-1 each set the four image bounds and viewing_cos_limit to the
    model's own u / v / view_cos of five points in view (five random ones, drawn again until the leftmost A and the rightmost B lie
    between the topmost C and the lowest D and the fifth, E, has the smallest view_cos), at the value itself or one ulp inside or outside; then one row per shape with
    the plain bounds, where the shape's threshold points and the th cases are counted."""
    rows = []
    for r in range(NBOUND_ROWS):
        shape = shapes[r % len(shapes)]
        sf, logS = shape_params(shape)
        while True:
            five = rng.choice(inview, 5, replace=False)
            five = five[np.argsort(rec0["u"][five])]
            A, B, mid = five[0], five[4], five[1:4]
            mid = mid[np.argsort(rec0["v"][mid])]
            C, Ept, D = mid
            va, vb, ve = rec0["v"][A], rec0["v"][B], rec0["v"][Ept]
            if rec0["u"][A] < rec0["u"][mid].min() and rec0["u"][mid].max() < rec0["u"][B] and \
                    rec0["v"][C] < min(va, vb, ve) and max(va, vb, ve) < rec0["v"][D] and \
                    rec0["view_cos"][Ept] < rec0["view_cos"][[A, B, C, D]].min():
                break
        bounds, want = [], []
        for b, (name, p) in enumerate(zip(BOUNDS, (A, B, C, D))):
            side = SIDES[(r + b) % 3]
            val = rec0["u" if b < 2 else "v"][p]
            lower = b % 2 == 0                                  # min_x, min_y: outside = the bound one ulp above the point
            step = {"at": 0, "inside": -1 if lower else 1, "outside": 1 if lower else -1}[side]
            bounds.append(up(val, step))
            want.append((name, side, int(p), (M.LEFT, M.RIGHT, M.TOP, M.BOTTOM)[b] if side == "outside" else M.IN_VIEW))
        side = SIDES[(r + 4) % 3]
        limit = up(rec0["view_cos"][Ept], {"at": 0, "inside": -1, "outside": 1}[side])
        want.append(("limit", side, int(Ept), M.VIEWCOS if side == "outside" else M.IN_VIEW))
        rows.append((dict(cam, bounds=tuple(bounds), viewing_cos_limit=limit, scale_factors=sf, log_scale_factor=logS),
                     TH3[(r // len(shapes)) % 3], shape))
        for name, side, p, code in want:
            E.case(name, side, r, p, code)
    for k, shape in enumerate(shapes * 3):                      # (three times: the base shape meets each of the three th values)
        sf, logS = shape_params(shape)
        rows.append((dict(cam, scale_factors=sf, log_scale_factor=logS), TH3[(k // len(shapes)) % 3], shape))
    return rows


def make(oracle, npoints=1000, nfeatures=900, seed=20):
    """The edge scene: dict with the frame (kps, desc, gp), every point (keys, pos, normal, min_dist, max_dist, pdesc, flags), the
    cameras ("cams": id -> (camera dict, th, shape)), "rows" (ids of the batched form, in order), "cases" and "refused"."""
    from orbhip import localmap
    sc = scenes.make(oracle, "640x480", npoints=npoints, nfeatures=nfeatures)
    w, h = sc["w"], sc["h"]
    rng = np.random.default_rng(seed)
    cam = dict(sc["cam"], mbf=f32(40.0))
    sc["cam"] = cam
    rec0, code0 = M.frustum(cam, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    inview = np.nonzero((code0 == M.IN_VIEW) & ((sc["flags"] & 2) == 0))[0]      # (a bad point is never tested)
    E = _Scene(sc)
    E.reach = {}
    E.reach["near/far tried"] = _near_far(E, cam, rng.permutation(inview), rng)
    tables, refused = {}, []
    for shape in SHAPES:
        sf, logS = shape_params(shape)
        try:
            tables[shape] = localmap.predict_scale_table(logS, shape[1])
        except Exception as e:                                  # the builder refuses what it cannot verify
            assert shape != BASE_SHAPE, e
            refused.append(shape)
            continue
        nth = shape[1] - 1
        E.reach["level %s tried, exact" % (shape,)] = _levels(E, cam, shape, tables[shape], rng.permutation(inview),
                                                              -(-FLOOR // nth) if nth else 0)
    # the base camera sees the base shape's threshold points
    for (kind, side, cid, idx, code, lv) in list(E.cases):
        if cid == BASE_SHAPE:
            E.case(kind, side, "base", idx, code, lv)
    E.reach["0.998 tried, found"] = _view_cos_998(E, cam, rng.permutation(inview), rng, w, h, cam["scale_factors"])
    pcz_cams = _pcz(E, int(inview[0]))
    shapes = [s for s in SHAPES if s not in refused]
    rows = _rows(E, cam, inview, rec0, rng, shapes)
    cams = {"base": (cam, f32(1.0), BASE_SHAPE)}
    cams.update({k: (c, f32(1.0), BASE_SHAPE) for k, c in pcz_cams.items()})
    row_ids = []
    for r, row in enumerate(rows):
        cams[r] = row
        row_ids.append(r)
    # the shape's threshold points are cases of every plain row of that shape; the 0.998 points are th cases of the base shape's
    first_plain = NBOUND_ROWS
    cases = []
    for c in E.cases:
        if isinstance(c[2], tuple):
            for r in row_ids[first_plain:]:
                if cams[r][2] == c[2]:
                    cases.append((c[0], c[1], r) + c[3:])
        else:
            cases.append(c)
    for r in row_ids[first_plain:]:
        if cams[r][2] == BASE_SHAPE:
            for j in E.planted:
                cases.append(("th", "%.9g" % cams[r][1], r, j, M.IN_VIEW, E.planted[j][3]))
    for r in row_ids[first_plain:]:
        if cams[r][2][1] == 1:                                  # one level: the table is empty, every point in view has level 0
            rec, code = M.frustum(cams[r][0], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
            for j in np.nonzero(code == M.IN_VIEW)[0][:FLOOR]:
                cases.append(("one level", "in view", r, int(j), M.IN_VIEW, 0))
    # the frame: the scene's features and one planted feature per 0.998 case, with the case's descriptor
    kps, desc = sc["kps"], sc["desc"]
    sf0 = cam["scale_factors"]
    extra = np.repeat(kps[:1], len(E.planted))
    planted = {}
    for n, (j, (u, v, dxy, lv)) in enumerate(E.planted.items()):
        off = PLANT * float(sf0[lv])
        extra["x"][n], extra["y"][n], extra["octave"][n] = u + dxy[0] * off, v + dxy[1] * off, lv
        planted[j] = len(kps) + n
    npts = len(E.pos)
    keys = (rng.permutation(npts).astype(np.uint64) + np.uint64(1)) * np.uint64(7919)
    flags = np.concatenate([sc["flags"], np.ones(npts - len(sc["flags"]), np.uint8)])
    out = dict(w=w, h=h, kps=np.concatenate([kps, extra]), desc=np.concatenate([desc, np.stack([E.desc[j] for j in E.planted])]),
               gp=sc["gp"], cam=cam, u_right=None, occupied=np.zeros(len(kps) + len(extra), np.uint8), keys=keys,
               pos=np.stack(E.pos), normal=np.stack(E.nrm), min_dist=np.array(E.mn, f32), max_dist=np.array(E.mx, f32),
               pdesc=np.stack(E.desc), flags=flags, cams=cams, rows=row_ids, first_plain=first_plain, cases=cases, planted=planted,
               refused=refused, shapes=shapes, tables=tables, reach=E.reach, name="edges")
    return out


def model_all(oracle, sc):
    """The model's answer for every camera of the scene over the whole point list, in the order of sc["keys"]:
    id -> (records, exit codes, n_to_match, nmatches, match, queries, qdesc).  Computed once per scene."""
    if "_model" not in sc:
        store = M.Store(len(sc["keys"]))
        store.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
        none = np.zeros(len(sc["keys"]), np.uint8)
        sc["_model"] = {cid: M.search_local_points(oracle, store, dict(cam), th, sc["keys"], none, sc["kps"], sc["desc"], sc["gp"], 0.8,
                                                   None, sc["occupied"]) for cid, (cam, th, shape) in sc["cams"].items()}
    return sc["_model"]


def verify(oracle, sc):
    """Every case got the exit code and level meant for it (model alone); the planted feature of every 0.998 / th case is matched
    exactly when the model's radius is 4.0 * th * scale factor; a floor on each tally.  Returns the tallies."""
    model = model_all(oracle, sc)
    tally = {}
    for kind, side, cid, idx, code, lv in sc["cases"]:
        rec, got = model[cid][0], model[cid][1]
        assert got[idx] == code, (kind, side, cid, idx, M.EXITS[got[idx]], M.EXITS[code])
        if code == M.IN_VIEW and lv is not None:
            assert rec["level"][idx] == lv, (kind, side, cid, idx, int(rec["level"][idx]), lv)
        if kind in ("0.998", "th"):
            cam, th, shape = sc["cams"][cid]
            sf = float(cam["scale_factors"][lv])
            wide = not f64(rec["view_cos"][idx]) > 0.998
            assert (kind == "th") or wide == (side == "below")
            r = float(model[cid][5]["radius"][idx])
            assert r == float(f32(M.radius(rec["view_cos"][idx], th) * f32(sf)))
            assert 2.5 * sf * float(th) < PLANT * sf < 4.0 * sf * float(th)
            assert (model[cid][4][sc["planted"][idx]] == idx) == wide, (kind, side, cid, idx)
            side = side + (" r=4.0" if wide else " r=2.5") if kind == "th" else side
        key = (kind if kind not in ("level", "clamp", "one level") else "%s %s" % (kind, sc["cams"][cid][2]), side)
        tally[key] = tally.get(key, 0) + 1
    for shape in sc["shapes"]:
        assert any(k[0] in ("level %s" % (shape,), "one level %s" % (shape,)) for k in tally), shape
    for (kind, side), n in tally.items():
        small = kind == "pcz" or kind.startswith("clamp") or kind == "th"
        if kind == "pcz":
            continue
        assert n >= (FLOOR_SMALL if small else FLOOR), (kind, side, n)
    assert sum(n for (kind, _), n in tally.items() if kind == "pcz") >= FLOOR_SMALL
    assert len({side.split(" r=")[0] for (kind, side) in tally if kind == "th"}) == 3
    assert all(any(k == ("th", "%.9g r=%s" % (t, r)) for k in tally) for t in TH3 for r in ("2.5", "4.0"))
    for a, b in zip(sc["rows"], sc["rows"][1:]):
        assert sc["cams"][a][2] != sc["cams"][b][2]
    return tally


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "vi-orb-slam-icra2018_amd"), os.path.join(here, "..", "oracle")]
    import orb_oracle_py as oracle
    oracle.build()
    sc = make(oracle)
    print(len(sc["keys"]), "points,", len(sc["kps"]), "features,", len(sc["rows"]), "rows; refused shapes:", sc["refused"] or "none")
    for k, v in sc["reach"].items():
        print("  reach:", k, v)
    for (kind, side), n in sorted(verify(oracle, sc).items()):
        print("  %-22s %-14s %d" % (kind, side, n))
