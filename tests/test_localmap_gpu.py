"""The resident map-point store and orbhip_search_local_points on the device against the independent model
(tests/localmap_model.py) and the oracle's window search: per-point records by bit pattern, n_to_match, match[], nmatches; equal
to orbhip_search_by_projection fed with the model's queries (old path = new path); the store's life cycle; order dependence; the
batched device form."""
import numpy as np
import pytest

import localmap_model as M
import localmap_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
FRAME = 77


def _cam_record(cam, th):
    from orbhip import localmap
    return localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                           cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], th)


class Rig:
    """One context with the scene's frame as a resident set and its points in the store and in the model's store."""

    def __init__(self, sc, max_points=4096, put=True):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.sc = sc
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.m = ORBmatcher(0.8, False, ctx=self.ex)
        self.m.put_set(FRAME, sc["kps"], sc["desc"], None, sc["gp"])
        self.lm = localmap.LocalMap(self.ex, max_points)
        self.model = M.Store(max_points)
        if put:
            self.put(np.arange(len(sc["keys"])))

    def put(self, idx, **over):
        a = {k: over.get(k, self.sc[k])[idx] if k not in over else over[k]
             for k in ("keys", "pos", "normal", "min_dist", "max_dist", "pdesc", "flags")}
        self.lm.put(a["keys"], a["pos"], a["normal"], a["min_dist"], a["max_dist"], a["pdesc"], a["flags"])
        self.model.put(a["keys"], a["pos"], a["normal"], a["min_dist"], a["max_dist"], a["pdesc"], a["flags"])

    def compare(self, oracle, keys, skip, th=1.0, frame=True, check_old_path=False):
        from orbhip import guided
        sc = self.sc
        got = self.lm.search(FRAME if frame else 0, len(sc["kps"]) if frame else 0, _cam_record(sc["cam"], th), keys, skip, 0.8,
                             sc["u_right"] if frame else None, sc["occupied"] if frame else None)
        rec, code, ntm, nm, match, q, qd = M.search_local_points(oracle, self.model, sc["cam"], th, keys, skip,
                                                                 sc["kps"] if frame else None, sc["desc"], sc["gp"], 0.8,
                                                                 sc["u_right"], sc["occupied"])
        pts = got[0]
        for f in ("u", "v", "proj_xr", "view_cos"):
            assert np.array_equal(pts[f].view(np.uint32), rec[f].view(np.uint32)), f
        assert np.array_equal(pts["level"], rec["level"]) and np.array_equal(pts["in_view"], rec["in_view"])
        assert got[1] == ntm and got[2] == nm and np.array_equal(got[3], match)
        if check_old_path and frame:
            on, om = guided.SearchByProjection(self.ex, sc["kps"], sc["desc"], sc["gp"], q, qd, sc["u_right"], sc["occupied"], True, 0.8,
                                               False, 100)
            assert on == got[2] and np.array_equal(om, got[3])
        return rec, code, ntm, nm, match

    def close(self):
        self.m.close()
        self.ex.close()


@pytest.mark.parametrize("name", list(scenes.SCENES))
def test_every_exit_and_level_bit_for_bit(oracle, name):
    sc = scenes.make(oracle, name)
    assert np.isfinite(sc["pos"]).all() and np.isfinite(sc["normal"]).all()
    d = np.linalg.norm(sc["pos"].astype(np.float64) - sc["cam"]["Ow"].astype(np.float64), axis=1)
    assert (d > 0).all()
    rig = Rig(sc)
    rng = np.random.default_rng(5)
    skip = (rng.random(len(sc["keys"])) < 0.05).astype(np.uint8)
    for th in (1.0, 3.0, 5.0):
        rec, code, ntm, nm, match = rig.compare(oracle, sc["keys"], skip, th, check_old_path=True)
        exits, levels = scenes.tallies(code, rec)
        print(name, "th", th, "n_to_match", ntm, "nmatches", nm, exits, levels)
        assert all(v >= scenes.FLOOR for v in exits.values()), exits
        assert all(v >= scenes.FLOOR for v in levels.values()), levels
        assert nm >= 100 and (code == M.NOT_TESTED).sum() >= scenes.FLOOR
        hi = rec["in_view"] == 1
        assert (hi & (rec["view_cos"] > 0.998)).sum() >= scenes.FLOOR and (hi & ~(rec["view_cos"] > 0.998)).sum() >= scenes.FLOOR
    rig.close()


def test_store_life_cycle(oracle):
    from orbhip import capi
    sc = scenes.make(oracle, "640x480", npoints=1200)
    keys = sc["keys"]
    rig = Rig(sc, max_points=1300)
    none = np.zeros(len(keys), np.uint8)
    assert rig.lm.info() == (1200, 1300)
    base = rig.compare(oracle, keys, none)
    # move some points: put again under the same keys
    rng = np.random.default_rng(9)
    moved = np.sort(rng.choice(1200, 300, replace=False))
    pos2 = sc["pos"][moved] + (rng.standard_normal((300, 3)) * 0.02).astype(f32)
    rig.put(moved, pos=pos2)
    assert rig.lm.info() == (1200, 1300)
    after = rig.compare(oracle, keys, none)
    assert not np.array_equal(after[0]["u"], base[0]["u"])
    # a point in view turns bad; points without observations gain their first (who may overwrite whom changes)
    inview = np.nonzero(after[0]["in_view"] == 1)[0]
    bad = inview[:40]
    unobs = np.nonzero(sc["flags"] == 0)[0]
    fl = sc["flags"].copy()
    fl[bad] |= 2
    fl[unobs] |= 1
    ch = np.unique(np.concatenate([bad, unobs]))
    rig.lm.update_flags(keys[ch], fl[ch])
    rig.model.update_flags(keys[ch], fl[ch])
    flagged = rig.compare(oracle, keys, none)
    assert flagged[2] == after[2] - 40 and (flagged[1][bad] == M.NOT_TESTED).all()
    # erase, keys the store never saw, skip bytes
    gone = inview[40:140]
    rig.lm.erase(keys[gone])
    rig.model.erase(keys[gone])
    assert rig.lm.info() == (1100, 1300)
    assert (rig.lm.slots(keys[gone]) == -1).all()
    strange = np.concatenate([keys, np.array([3, 5, 2 ** 63 + 11], np.uint64)])
    skip = np.zeros(len(strange), np.uint8)
    skip[inview[140:200]] = 1
    e = rig.compare(oracle, strange, skip, 3.0)
    assert (e[1][gone] == M.NOT_TESTED).all() and (e[1][-3:] == M.NOT_TESTED).all() and (e[1][inview[140:200]] == M.NOT_TESTED).all()
    # the slots of erased points are used again
    rig.put(gone)
    assert rig.lm.info() == (1200, 1300) and (rig.lm.slots(keys[gone]) >= 0).all()
    rig.compare(oracle, strange, skip)
    # max_points reached: an error, and the store as it was
    extra = np.arange(101, dtype=np.uint64) + np.uint64(10 ** 9)
    z3, z1 = np.zeros((101, 3), f32), np.ones(101, f32)
    mixed = np.concatenate([keys[:5], extra])          # five updates and 101 new points: one too many
    with pytest.raises(capi.OrbHipError, match="max_points"):
        rig.lm.put(mixed, np.zeros((106, 3), f32), np.zeros((106, 3), f32), np.ones(106, f32), np.ones(106, f32),
                   np.zeros((106, 32), np.uint8), np.zeros(106, np.uint8))
    assert rig.lm.info() == (1200, 1300) and (rig.lm.slots(extra) == -1).all()
    rig.compare(oracle, strange, skip)
    rig.lm.put(extra[:100], z3[:100], z3[:100], z1[:100], z1[:100], np.zeros((100, 32), np.uint8), np.zeros(100, np.uint8))
    assert rig.lm.info() == (1300, 1300)
    with pytest.raises(capi.OrbHipError):
        rig.lm.put(keys[:2][[0, 0]], z3[:2], z3[:2], z1[:2], z1[:2], np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8))   # a key twice
    with pytest.raises(capi.OrbHipError):
        rig.lm.update_flags(np.array([4242], np.uint64), np.zeros(1, np.uint8))
    # empty local map; a frame without features; an unknown frame
    got = rig.lm.search(FRAME, len(sc["kps"]), _cam_record(sc["cam"], 1.0), np.zeros(0, np.uint64), np.zeros(0, np.uint8))
    assert got[1] == 0 and got[2] == 0 and (got[3] == -1).all() and len(got[0]) == 0
    rig.compare(oracle, strange, skip, frame=False)
    with pytest.raises(capi.OrbHipError, match="unknown set"):
        rig.lm.search(12345, 10, _cam_record(sc["cam"], 1.0), keys, none)
    rig.lm.clear()
    assert rig.lm.info() == (0, 1300)
    got = rig.lm.search(FRAME, len(sc["kps"]), _cam_record(sc["cam"], 1.0), keys, none)
    assert got[1] == 0 and got[2] == 0 and (got[0]["in_view"] == 0).all()
    rig.close()


@pytest.mark.parametrize("observed", [True, False])
def test_points_competing_for_one_feature_in_every_order(oracle, observed):
    """Several points project onto the same feature with the same descriptor: which one the feature ends up with depends on the
    order of the list and on whether the earlier point has observations (ref: src/ORBmatcher.cc:87-89, :123)."""
    sc = scenes.make(oracle, "640x480", npoints=600)
    rng = np.random.default_rng(17)
    rec, code = M.frustum(sc["cam"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    src = np.nonzero(code == M.IN_VIEW)[0][:120]
    # four copies of each: same geometry, a few bits of the descriptor flipped, keys of their own
    idx = np.repeat(src, 4)
    pd = sc["pdesc"][idx].copy()
    for j in range(len(idx)):
        for b in rng.integers(0, 256, j % 4):
            pd[j, b >> 3] ^= np.uint8(1 << (b & 7))
    keys = np.arange(1, len(idx) + 1, dtype=np.uint64) * np.uint64(13)
    flags = np.full(len(idx), 1 if observed else 0, np.uint8)
    if not observed:
        flags[rng.random(len(idx)) < 0.3] = 1
    rig = Rig(sc, put=False)
    rig.lm.put(keys, sc["pos"][idx], sc["normal"][idx], sc["min_dist"][idx], sc["max_dist"][idx], pd, flags)
    rig.model.put(keys, sc["pos"][idx], sc["normal"][idx], sc["min_dist"][idx], sc["max_dist"][idx], pd, flags)
    seen = set()
    for trial in range(6):
        order = np.arange(len(idx)) if trial == 0 else rng.permutation(len(idx))
        r = rig.compare(oracle, keys[order], np.zeros(len(idx), np.uint8), 3.0, check_old_path=True)
        assert r[3] >= 60
        winners = keys[order][r[4][r[4] >= 0]]
        seen.add(winners.tobytes())
    assert len(seen) > 1     # the order matters in this scene
    rig.close()


@pytest.mark.parametrize("B", [1, 8, 64])
def test_device_form_equals_single_calls(oracle, B):
    import hiprt
    from orbhip import capi, localmap
    from orbhip.capi import check
    sc = scenes.make(oracle, "1241x376_stereo", npoints=1500)
    rig = Rig(sc)
    rng = np.random.default_rng(23 + B)
    n, cap, nqmax = len(sc["kps"]), len(sc["kps"]) + 13, 1500
    capq = nqmax + 7
    cams = np.zeros(B, localmap.CAMERA_DTYPE)
    keys = np.zeros((B, capq), np.uint64)
    skip = np.zeros((B, capq), np.uint8)
    nq = np.zeros(B, np.int32)
    for b in range(B):
        R, t, Ow = scenes.pose(rng)
        cams[b] = _cam_record(dict(sc["cam"], Rcw=R, tcw=t, Ow=Ow), (1.0, 3.0, 5.0)[b % 3])[0]
        nq[b] = nqmax - 37 * (b % 5)
        keys[b, :nq[b]] = rng.permutation(sc["keys"])[:nq[b]]
        skip[b, :nq[b]] = rng.random(nq[b]) < 0.05
    slots = rig.lm.slots(keys.ravel()).reshape(B, capq)
    kps = np.zeros((B, cap), capi.KP_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    ur = np.full((B, cap), -1, f32)
    occ = np.zeros((B, cap), np.uint8)
    kps[:, :n], desc[:, :n], ur[:, :n], occ[:, :n] = sc["kps"], sc["desc"], sc["u_right"], sc["occupied"]
    D = hiprt.DevBuf
    d = dict(kps=D.from_numpy(kps), desc=D.from_numpy(desc), cnt=D.from_numpy(np.full(B, n, np.int32)), ur=D.from_numpy(ur),
             occ=D.from_numpy(occ), off=D(B * (64 * 48 + 1) * 4), idx=D(B * cap * 4), cam=D.from_numpy(rig.lm.prepare(cams)),
             slots=D.from_numpy(slots), skip=D.from_numpy(skip), nq=D.from_numpy(nq), pts=D(B * capq * 24), ntm=D(B * 4),
             m=D(B * cap * 4), nm=D(B * 4))
    gp = sc["gp"]
    L, h = rig.ex._L, rig.ex.handle
    check(L.orbhip_grid_build_device(h, d["kps"].ptr, d["cnt"].ptr, cap, B, gp[0], gp[1], gp[2], gp[3], d["off"].ptr, d["idx"].ptr), h,
          "grid")
    for rep in range(2):     # twice: n_to_match is set, not accumulated
        check(L.orbhip_search_local_points_device(h, d["kps"].ptr, d["desc"].ptr, d["cnt"].ptr, cap, B, d["ur"].ptr, d["occ"].ptr, gp[0],
                                                  gp[1], gp[2], gp[3], d["off"].ptr, d["idx"].ptr, d["cam"].ptr, d["slots"].ptr,
                                                  d["skip"].ptr, d["nq"].ptr, capq, 0.8, d["pts"].ptr, d["ntm"].ptr, d["m"].ptr,
                                                  d["nm"].ptr), h, "orbhip_search_local_points_device")
    rig.ex.sync()
    pts = d["pts"].to_numpy(localmap.POINT_DTYPE, (B, capq))
    ntm, nm, m = d["ntm"].to_numpy(np.int32, (B,)), d["nm"].to_numpy(np.int32, (B,)), d["m"].to_numpy(np.int32, (B, cap))
    for b in range(B):
        one = rig.lm.search(FRAME, n, cams[b:b + 1], keys[b, :nq[b]], skip[b, :nq[b]], 0.8, sc["u_right"], sc["occupied"])
        assert pts[b, :nq[b]].tobytes() == one[0].tobytes() and ntm[b] == one[1] and nm[b] == one[2]
        assert np.array_equal(m[b, :n], one[3]) and (m[b, n:] == -1).all()
        assert one[1] > 0 and one[2] > 0     # (not a comparison of empty results)
    if B == 1:
        rig.compare(oracle, keys[0, :nq[0]], skip[0, :nq[0]], 1.0)
    rig.close()
    for x in d.values():
        x.free()
