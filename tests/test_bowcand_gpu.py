"""orbhip_search_by_bow_candidates on the device against the model of the two SearchByBoW loops (tests/bowcand_model.py): exact
equality of every output on the scenes of tests/bowcand_scenes.py, built to reach each path and edge of the kernels
(csrc/bow_match_dev.h: side-2 nodes of <= 128, <= 4096 and more features, side-1 chunks of 64; csrc/k_bowcand.hip: four pairs per
block, one wave per candidate).  Every call is also compared row by row with orbhip_search_by_bow_sets on the same pair, given
validity bytes derived from the same rows."""
import numpy as np
import pytest

import bowcand_model as M
import bowcand_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_CAPACITY = r"\(-1\)", r"\(-3\)"


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    yield e
    e.close()


class Rig:
    """A store, a key-frame table and resident sets beside the model's sides.  A side becomes a set (and, for a key frame, a row
    and its points) under one key; the rig remembers which point every row entry named when the row was put, so `view` gives the
    side as the device sees it now: an entry counts iff that very point is still in the store and not bad."""

    def __init__(self, ex, max_points=16384, max_kfs=24, max_row=4200):
        from orbhip import localmap
        from orbhip.extractor import ORBmatcher
        self.ex = ex
        self.lm = localmap.LocalMap(ex, max_points, max_kfs, max_row)
        self.m = ORBmatcher(0.75, True, ctx=ex)
        self.m.drop_set(0)
        self.keys, self.sides, self.rows = {}, {}, {}     # id(side) -> key; key -> side; key -> [(point key, serial) or None]
        self.world = {}                                   # point key -> [serial, bad, pos]
        self.next_key, self.next_point, self.serial = 100, 1000, 0

    def put_points(self, keys, pts):
        n = len(keys)
        if n == 0:
            return
        pos = np.asarray([p.pos for p in pts], f32).reshape(n, 3)
        self.lm.put(np.asarray(keys, np.uint64), pos, np.zeros((n, 3), f32), np.ones(n, f32), np.ones(n, f32), np.zeros((n, 32), np.uint8),
                    np.asarray([3 if p.bad else 1 for p in pts], np.uint8))
        for k, p in zip(keys, pts):
            self.serial += 1
            self.world[int(k)] = [self.serial, p.bad, p.pos]

    def add(self, side, kf=True):
        if id(side) in self.keys:
            return self.keys[id(side)]
        from orbhip.capi import KP_DTYPE
        key = self.next_key
        self.next_key += 7
        n = len(side["desc"])
        kps = np.zeros(n, KP_DTYPE)
        kps["x"], kps["y"], kps["angle"], kps["octave"] = side["x"], side["y"], side["angle"], side["octave"]
        self.m.put_set(key, kps, side["desc"], M.csr(side["fv"]))
        self.keys[id(side)], self.sides[key] = key, side
        if kf:
            have = [i for i, p in enumerate(side["points"]) if p is not None]
            pk = np.zeros(n, np.uint64)
            pk[have] = np.arange(self.next_point, self.next_point + len(have), dtype=np.uint64)
            self.next_point += len(have)
            self.put_points([int(pk[i]) for i in have], [side["points"][i] for i in have])
            self.lm.kf_put(key, pk)
            self.rows[key] = [None if k == 0 else (int(k), self.world[int(k)][0]) for k in pk]
        return key

    def view(self, side):
        key = self.keys[id(side)]
        if key not in self.rows:
            return side
        pts = []
        for e in self.rows[key]:
            w = self.world.get(e[0]) if e else None
            pts.append(M.Point(w[1], w[2]) if w and w[0] == e[1] else None)
        return dict(side, points=pts)

    def point_keys(self, side):
        return [e[0] for e in self.rows[self.keys[id(side)]] if e]

    # edits of the store, mirrored
    def erase(self, keys):
        self.lm.erase(np.asarray(keys, np.uint64))
        for k in keys:
            self.world.pop(int(k), None)

    def set_bad(self, keys, bad=True):
        self.lm.update_flags(np.asarray(keys, np.uint64), np.full(len(keys), 3 if bad else 1, np.uint8))
        for k in keys:
            self.world[int(k)][1] = bad

    def clear(self):
        self.lm.clear()
        self.world.clear()


def _raises(code, f, *a, **kw):
    from orbhip import capi
    with pytest.raises(capi.OrbHipError, match=code) as e:
        f(*a, **kw)
    return e.value


def _untouched(outs):
    return all((np.asarray(o) == -7).all() for o in outs)


def _single(rig, mode, fixed, cand, th, ratio, ori):
    """orbhip_search_by_bow_sets on the pair, validity bytes from the rig's view of the rows: the row of the batched call"""
    s1, s2 = (cand, fixed) if mode == 0 else (fixed, cand)
    v1 = M.valid_bytes(rig.view(s1))
    v2 = None if mode == 0 else M.valid_bytes(rig.view(s2))
    rig.m.TH_LOW, rig.m.mfNNratio, rig.m.mbCheckOrientation = th, ratio, ori
    nm, m12, m21 = rig.m.SearchByBoW_sets(rig.keys[id(s1)], v1, len(v1), rig.keys[id(s2)], v2, len(s2["desc"]), kf_kf=(mode == 1))
    return [int(x) for x in (m21 if mode == 0 else m12)], nm


def check(rig, mode, scene, gather=None, single=True, **over):
    """The call against the model -- every output -- and against the single call per pair."""
    fixed, cands, p = scene
    p = dict(p, **over)
    th, ratio, ori = p.get("th", 50), p.get("nnratio", 0.75), p.get("check_ori", True)
    fk = rig.add(fixed, kf=(mode == 1))
    ck = [rig.add(c) for c in cands]
    want = M.candidates(mode, rig.view(fixed), [rig.view(c) for c in cands], th, ratio, ori, gather)
    got = rig.lm.search_by_bow_candidates(mode, fk, fk if mode == 1 else 0, len(fixed["desc"]), [(k, k) for k in ck], th, ratio, ori, gather)
    assert [[int(x) for x in r] for r in got[0]] == want["matches"]
    assert [int(x) for x in got[1]] == want["nmatches"]
    if gather is not None:
        g = got[2]
        assert [int(x) for x in g["off"]] == want["off"]
        assert [int(x) for x in g["kp_idx"]] == want["kp_idx"] and [int(x) for x in g["kf_idx"]] == want["kf_idx"]
        assert g["P3Dw"].tobytes() == np.asarray(want["P3Dw"], f32).reshape(-1, 3).tobytes()
        assert g["P2D"].tobytes() == np.asarray(want["P2D"], f32).reshape(-1, 2).tobytes()
        assert g["max_err"].tobytes() == np.asarray(want["max_err"], f32).tobytes()
    if single:
        for k, c in enumerate(cands):
            assert _single(rig, mode, fixed, c, th, ratio, ori) == (want["matches"][k], want["nmatches"][k])
    return want


MODES = [0, 1]


# ---- node sizes ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n2", [0, 1, 64, 65, 128, 129, 4097])
def test_side2_node_sizes(ex, mode, n2):
    rig = Rig(ex)
    check(rig, mode, S.node_sizes(mode, n2))
    want = check(rig, mode, S.node_sizes(mode, n2, seed=1), check_ori=False)
    assert n2 == 0 or want["nmatches"][0] > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n1", [64, 65])
def test_side1_chunk_edge(ex, mode, n1):
    rig = Rig(ex)
    check(rig, mode, S.node_sizes(mode, 5, n1))
    check(rig, mode, S.node_sizes(mode, 129, n1), check_ori=False)


# ---- K and the pairs table ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [1, 2, 4, 5, 9])
def test_batches_straddle_blocks(ex, mode, K):
    want = check(Rig(ex), mode, S.batch(mode, K))
    assert sum(want["nmatches"]) > 0


@pytest.mark.parametrize("mode", MODES)
def test_candidate_twice_disjoint_and_none(ex, mode):
    rig = Rig(ex)
    want = check(rig, mode, S.twice(mode))
    assert want["matches"][0] == want["matches"][2] and sum(want["nmatches"]) > 0
    want = check(rig, mode, S.disjoint(mode))
    assert want["nmatches"][1] == 0 and all(x == -1 for x in want["matches"][1])
    fixed, cands, _ = S.disjoint(mode)      # a call in which NO candidate shares a node
    check(rig, mode, (fixed, [cands[1], cands[1]], {}), gather=(0, S.SIGMA2, 5.991) if mode == 0 else None)
    # K == 0: ORBHIP_OK, nothing written
    fk = rig.keys[id(fixed)]
    got = rig.lm.search_by_bow_candidates(mode, fk, fk if mode == 1 else 0, 7, [])
    assert got[0].shape == (0, 7) and len(got[1]) == 0
    L, h = rig.lm._L, ex.handle
    probe = np.full(8, -7, np.int32)
    from orbhip.capi import _p
    assert L.orbhip_search_by_bow_candidates(h, mode, 12345, 0, None, 0, 50, f32(0.75), 1, _p(probe), _p(probe), 0, None, 0, f32(0), None,
                                             None, None, None, None, None, 0, None) == 0
    assert (probe == -7).all()


# ---- validity through the rows ----
@pytest.mark.parametrize("mode", MODES)
def test_all_invalid_row(ex, mode):
    want = check(Rig(ex), mode, S.all_invalid(mode))
    assert want["nmatches"] == [0]


@pytest.mark.parametrize("mode", MODES)
def test_stale_and_bad_entries(ex, mode):
    rig = Rig(ex)
    scene = S.batch(mode, 4, seed=21)
    fixed, cands, _ = scene
    g = (2, S.SIGMA2, 5.991) if mode == 0 else None
    base = check(rig, mode, scene, gather=g)
    assert sum(base["nmatches"]) > 0
    rng = np.random.default_rng(5)
    sides = cands + ([fixed] if mode == 1 else [])         # mode 1: the fixed row's validity too

    def matched():
        return M.candidates(mode, rig.view(fixed), [rig.view(c) for c in cands], check_ori=False)["matches"]
    before = matched()
    # bad points
    bad = [k for s in sides for k in rng.choice(rig.point_keys(s), 4, replace=False)]
    rig.set_bad(bad)
    check(rig, mode, scene, gather=g)
    # erased points: their entries are stale
    gone = [k for s in sides for k in rng.choice(rig.point_keys(s), 6, replace=False) if k in rig.world]
    freed = sorted(int(s) for s in rig.lm.slots(gone))
    rig.erase(gone)
    check(rig, mode, scene, gather=g)
    # slot re-use: new points take the freed slots, the old entries still name the old generation
    new = [900000 + i for i in range(len(gone))]
    rig.put_points(new, [M.Point(False, (f32(1), f32(2), f32(3)))] * len(new))
    assert sorted(int(s) for s in rig.lm.slots(new)) == freed
    check(rig, mode, scene, gather=g)
    # ... and the same KEY put again is another point to the row as well
    rig.put_points(gone[:3], [M.Point(False, (f32(4), f32(5), f32(6)))] * 3)
    check(rig, mode, scene, gather=g)
    assert matched() != before
    # orbhip_map_clear: every entry is stale
    rig.clear()
    want = check(rig, mode, scene, gather=g)
    assert want["nmatches"] == [0] * 4


# ---- thresholds and ties ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["threshold", "ratio_equal", "ratio_next", "tie", "claimed"])
def test_thresholds_and_ties(ex, mode, name):
    scene = {"threshold": S.threshold, "ratio_equal": S.ratio_equal, "ratio_next": lambda m: S.ratio_equal(m, 5), "tie": S.tie,
             "claimed": S.claimed}[name](mode)
    want = check(Rig(ex), mode, scene, check_ori=False)
    expect = {"threshold": 1 if mode == 0 else 0, "ratio_equal": 0, "ratio_next": 1, "tie": 1, "claimed": 2}[name]
    assert want["nmatches"] == [expect]


# ---- rotation ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,on,off", [("rot_two_bins", 5, 5), ("rot_second_below_tenth", 11, 12), ("rot_bin_30", 10, 11)])
def test_rotation(ex, mode, name, on, off):
    rig = Rig(ex)
    scene = getattr(S, name)(mode)
    assert check(rig, mode, scene, check_ori=True)["nmatches"] == [on]
    assert check(rig, mode, scene, check_ori=False)["nmatches"] == [off]


# ---- the PnPsolver arrays (mode 0) ----
def test_gather_min_matches_cap_and_octaves(ex):
    rig = Rig(ex)
    scene = S.gather_scene()
    for mm, off in ((6, [0, 6, 6, 12]), (7, [0, 0, 0, 0]), (5, [0, 6, 11, 17])):
        want = check(rig, 0, scene, gather=(mm, S.SIGMA2, 5.991))
        assert want["off"] == off
    assert {int(scene[0]["octave"][i]) for i in want["kp_idx"]} == {0, S.NLEVELS - 1}
    check(rig, 0, scene)                                    # all gather pointers NULL
    fk, ck = rig.keys[id(scene[0])], [rig.keys[id(c)] for c in scene[1]]
    args = (0, fk, 0, len(scene[0]["desc"]), [(k, k) for k in ck])
    got = rig.lm.search_by_bow_candidates(*args, gather=(5, S.SIGMA2, 5.991), cap=17)     # exactly enough
    assert len(got[2]["kp_idx"]) == 17
    e = _raises(E_CAPACITY, rig.lm.search_by_bow_candidates, *args, gather=(5, S.SIGMA2, 5.991), cap=16)   # one short
    assert e.total == 17 and _untouched(e.outputs)
    check(rig, 0, scene, gather=(5, S.SIGMA2, 5.991))       # the context is usable afterwards
    # a frame octave outside the per-level table
    e = _raises(E_ARG, rig.lm.search_by_bow_candidates, *args, gather=(5, S.SIGMA2[:S.NLEVELS - 1], 5.991))
    assert _untouched(e.outputs)


# ---- errors: nothing written, the context usable ----
@pytest.mark.parametrize("mode", MODES)
def test_errors_leave_outputs_and_context(ex, mode):
    rig = Rig(ex)
    scene = S.batch(mode, 2, seed=3)
    check(rig, mode, scene)
    fixed, cands, _ = scene
    fk, ck = rig.keys[id(fixed)], [rig.keys[id(c)] for c in cands]
    n = len(fixed["desc"])
    rk = fk if mode == 1 else 0
    g = (1, S.SIGMA2, 5.991) if mode == 0 else None
    call = rig.lm.search_by_bow_candidates
    for bad in ([(ck[0], ck[0]), (55555, ck[1])],            # an unknown set key
                [(ck[0], ck[0]), (ck[1], 55555)],            # an unknown row key
                [(ck[0], ck[1])] if len(cands[0]["desc"]) != len(cands[1]["desc"]) else None):   # a row of another length than the set
        if bad is None:
            continue
        e = _raises(E_ARG, call, mode, fk, rk, n, bad, gather=g)
        assert _untouched(e.outputs)
    assert len(cands[0]["desc"]) != len(cands[1]["desc"])
    e = _raises(E_ARG, call, mode, 55555, rk, n, [(k, k) for k in ck], gather=g)    # the fixed set unknown
    assert _untouched(e.outputs)
    if mode == 1:
        e = _raises(E_ARG, call, mode, fk, 55555, n, [(k, k) for k in ck])          # the fixed row unknown
        assert _untouched(e.outputs)
        e = _raises(E_ARG, call, mode, fk, ck[0], n, [(k, k) for k in ck])          # the fixed row of another length
        assert _untouched(e.outputs)
        e = _raises(E_ARG, call, mode, fk, rk, n, [(k, k) for k in ck], gather=(1, S.SIGMA2, 5.991))   # gather outputs in mode 1
        assert _untouched(e.outputs)
    e = _raises(E_ARG, call, 2, fk, rk, n, [(k, k) for k in ck])                    # no such mode
    assert _untouched(e.outputs)
    check(rig, mode, scene, gather=g)
    # more distinct sets than the limit in force: four candidates and the fixed side against a limit of four
    big = S.batch(mode, 4, seed=8)
    check(rig, mode, big)
    assert rig.m.set_limit(4) == 4
    try:
        bfk, bck = rig.keys[id(big[0])], [rig.keys[id(c)] for c in big[1]]
        e = _raises(E_ARG, call, mode, bfk, bfk if mode == 1 else 0, len(big[0]["desc"]), [(k, k) for k in bck])
        assert "set limit" in str(e) and _untouched(e.outputs)
    finally:
        assert rig.m.set_limit(96) == 96
    check(Rig(ex), mode, big)        # (the limit of four evicted sets: a fresh rig puts them again)
