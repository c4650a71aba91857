"""orbhip_fuse_sim3 / orbhip_search_loop_points / orbhip_map_kf_set_batch on the device.  Queries as 32-byte records, best_idx,
best_dist, n_active, match, nmatches and keys_out are compared by bit pattern against the independent model
(tests/loopfuse_model.py) and against the path that existed before them: the model's queries and the points' descriptors uploaded to
orbhip_window_best_set without a gate, respectively to orbhip_search_by_projection, which run none of the new kernels.
tests/test_loopfuse_model.py shows on the CPU that the scenes contain what these tests rely on."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as FM
import loopfuse_model as LM
import loopfuse_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE, E_CAPACITY = -1, -2, -3
OWN_ROW = 0x840


def _target_record(T, **kw):
    from orbhip import localmap
    cam = T["cam"]
    rec = localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                          cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], T["th"])
    for k, v in kw.items():
        rec[k] = v
    return localmap.fuse_target(T["key"], rec, T["sig"])


class Rig:
    """One context: the scene's target sets (with a grid), its points in the store, the targets' rows and the loop rows in the
    key-frame table.  The scene's stale points are erased after the rows were put, and the new points take their slots."""

    def __init__(self, sc, max_points=1024, max_kfs=16, max_row=512, rows=None):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.sc = sc
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.m = ORBmatcher(0.8, True, ctx=self.ex)
        for key, (kps, desc) in sc["sets"].items():
            self.m.put_set(key, kps, desc, None, sc["targets"][0]["gp"])
        self.lm = localmap.LocalMap(self.ex, max_points, max_kfs, max_row)
        self.lm.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
        for key, r in {**sc["rows"], **sc.get("loop_rows", {}), **(rows or {})}.items():
            self.lm.kf_put(key, r)
        if len(sc["stale"]):
            gone = sc["keys"][sc["stale"]]
            old = self.lm.slots(gone)
            self.lm.erase(gone)
            self.lm.put(*S.fresh_points(sc))
            new = self.lm.slots(sc["fresh_keys"])
            assert set(new) == set(old) and (new >= 0).all()           # the rows' stale entries name slots that hold list points now
            self.old_slot = dict(zip(gone.tolist(), old.tolist()))      # key that left -> the slot it had
            self.fresh_in = dict(zip(new.tolist(), sc["fresh_keys"].tolist()))   # slot -> the new point in it
        self.model = S.model_store(sc)

    def records(self, which):
        return np.concatenate([_target_record(self.sc["targets"][k]) for k in which])

    def sim3(self, oracle, which, n=None, rows=True, want_queries=True):
        from orbhip import guided
        sc = self.sc
        keys = sc["loop"] if n is None else sc["loop"][:n]
        row_keys = list(sc.get("row_keys") or S.ROWS)
        rk = np.array([row_keys[k] for k in which], np.uint64) if rows else None
        gq, gbi, gbd, gna = self.lm.fuse_sim3(self.records(which), rk, keys, want_queries)
        T = [sc["targets"][k] for k in which]
        want = LM.fuse_sim3(oracle, self.model, T, [sc["rows"].get(int(r)) if rows and r else None for r in (rk if rows else [0] * len(T))], keys)
        for j, (q, code, qd, na, bi, bd) in enumerate(want):
            if gq is not None:
                assert gq[j].tobytes() == q.tobytes(), (which[j], np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(gq[j], q)])[0])
            assert gna[j] == na and np.array_equal(gbi[j], bi) and np.array_equal(gbd[j], bd), which[j]
            obi, obd = guided.WindowBestSet(self.ex, T[j]["key"], q, qd, None, None)      # the old path: no gate
            assert np.array_equal(obi, gbi[j]) and np.array_equal(obd, gbd[j])
        return want

    def loop_points(self, oracle, T, loop_rows, matched, cap=512, th_high=LM.TH_LOW, want_queries=True):
        from orbhip import guided
        kk = np.array(list(loop_rows), np.uint64)
        keys, gq, gna, gnm, gmatch = self.lm.search_loop_points(_target_record(T), len(T["kps"]), kk, matched, cap, th_high, want_queries)
        wkeys, q, code, qd, na, nm, match = LM.search_loop_points(oracle, self.model, T, list(loop_rows.values()), matched, th_high)
        assert keys.tobytes() == wkeys.tobytes() and np.array_equal(keys, self.lm.collect(kk, cap))
        if gq is not None:
            assert gq.tobytes() == q.tobytes(), np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(gq, q)])[0]
        assert gna == na and gnm == nm and gmatch.tobytes() == match.tobytes()
        occ = None if matched is None else (np.asarray(matched) != 0).astype(np.uint8)
        onm, omatch = guided.SearchByProjection(self.ex, T["kps"], T["desc"], T["gp"], q, qd, None, occ, use_ratio=False, check_ori=False,
                                                th_high=th_high)                           # the old path
        assert onm == gnm and np.array_equal(omatch, gmatch)
        return keys, code, nm, match

    def close(self):
        self.m.close()
        self.ex.close()


@pytest.fixture(scope="module")
def main_scene():
    return S.make()


def test_main_scene_bit_for_bit(oracle, main_scene):
    rig = Rig(main_scene)
    out = rig.sim3(oracle, range(5))                    # five records over four sets of four sizes, one set twice, one without a row
    assert sum(int((o[5] <= LM.TH_LOW).sum()) for o in out) >= 100 and (out[1][1] == LM.SKIPPED).sum() >= 100
    codes = np.stack([o[1] for o in out])
    assert ((codes == LM.SKIPPED).any(axis=0) & (codes == LM.ACTIVE).any(axis=0)).sum() >= 5   # held here, free there
    # the stale entries of the first target's row name slots of list points: those take part
    pos = {int(k): i for i, k in enumerate(main_scene["loop"])}
    active = 0
    for k, row_key in enumerate(S.ROWS):
        if row_key:
            row = set(main_scene["rows"][row_key].tolist())
            took = [pos[rig.fresh_in[slot]] for key, slot in rig.old_slot.items() if key in row]
            assert len(took) >= 2 and (codes[k][took] != LM.SKIPPED).all()
            active += int((codes[k][took] == LM.ACTIVE).sum())
    assert active >= 4
    rig.sim3(oracle, [1])                               # K = 1
    rig.sim3(oracle, [0, 3])                            # K = 2: the same set under two similarities
    rig.sim3(oracle, [2])                               # the target without a row alone: no held pass at all
    rig.sim3(oracle, [3, 2, 0], rows=False)             # target_row_keys NULL
    rig.sim3(oracle, range(5), want_queries=False)      # the queries stay on the device
    rig.close()


def test_list_lengths_at_wave_and_block_edges(oracle, main_scene):
    """1, 63, 64, 65, 255, 256, 257 points: the ballot count of one wave, of a block and of the block after it; the last 16-lane row
    of the search; K = 1, 2 and 5."""
    rig = Rig(main_scene)
    active = 0
    for n in S.SIZES:
        for which in ([0], [0, 3], range(5)):
            active += sum(o[3] for o in rig.sim3(oracle, which, n=n))
    assert active > 1500
    rig.close()


def test_edge_scene(oracle):
    sc = S.edge_scene()
    rig = Rig(sc)
    (q, code, qd, na, bi, bd), = rig.sim3(oracle, [0])
    ix = sc["ix"]
    for case, want in S.EDGE_EXPECT.items():
        assert (code[ix[case]] != LM.ACTIVE) if want is None else (code[ix[case]] == want), case
    (q2, code2, _, _, _, _), = rig.sim3(oracle, [0], rows=False)      # the held point takes part now
    assert code2[ix["held"]] == LM.ACTIVE
    rig.close()


def test_marks_are_clear_afterwards(oracle, main_scene):
    """A following orbhip_fuse_collect, which marks the target's own row, gives its known answer; so does the vote."""
    sc = main_scene
    own = np.concatenate([sc["keys"][5:200:7], np.zeros(3, np.uint64)])
    rig = Rig(sc, rows={OWN_ROW: own})
    T = sc["targets"][0]
    kk = np.array(S.LOOP_ROWS, np.uint64)

    def collect():
        keys, gq, gbi, gbd, gna = rig.lm.fuse_collect(_target_record(T), OWN_ROW, kk, 512, None)
        held = {int(k) for k in own if int(k) in rig.model.pts}          # IsInKeyFrame: the row's points, bad ones included
        skip = np.array([int(k) in held for k in keys], np.uint8)
        q, code, qd, na, bi, bd = FM.fuse(oracle, rig.model, T, T["th"], keys, skip)
        assert np.array_equal(keys, FM.collect(rig.model, list(sc["loop_rows"].values())))
        assert gq.tobytes() == q.tobytes() and gna == na and np.array_equal(gbi, bi) and np.array_equal(gbd, bd)
        return na

    before = rig.lm.vote(sc["keys"][::3])
    assert collect() >= 50
    rig.sim3(oracle, range(5))
    assert collect() >= 50
    rig.loop_points(oracle, T, sc["loop_rows"], sc["matched"])
    assert collect() >= 50
    after = rig.lm.vote(sc["keys"][::3])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[1].sum() > 50
    rig.close()


def test_search_loop_points(oracle, main_scene):
    from orbhip import capi
    sc = main_scene
    rig = Rig(sc)
    T = sc["targets"][0]
    keys, code, nm, match = rig.loop_points(oracle, T, sc["loop_rows"], sc["matched"])
    assert len(keys) >= 200 and nm >= 10 and (code == LM.SKIPPED).sum() >= 3
    rig.loop_points(oracle, T, sc["loop_rows"], None)                                      # vpMatched all NULL
    rig.loop_points(oracle, T, sc["loop_rows"], sc["matched"], th_high=100, want_queries=False)
    rig.loop_points(oracle, sc["targets"][2], sc["loop_rows"], None)                       # a set of one feature
    rig.loop_points(oracle, sc["targets"][4], {S.LOOP_ROWS[1]: sc["loop_rows"][S.LOOP_ROWS[1]]}, None)
    # too little room: the first cap keys, the number, nothing else
    with pytest.raises(capi.OrbHipError) as e:
        rig.lm.search_loop_points(_target_record(T), len(T["kps"]), np.array(S.LOOP_ROWS, np.uint64), sc["matched"], 100)
    assert e.value.total == len(keys) and np.array_equal(e.value.partial, keys[:100])
    # an empty list of key frames, and rows that hold nothing
    k0, q0, na0, nm0, m0 = rig.lm.search_loop_points(_target_record(T), len(T["kps"]), np.zeros(0, np.uint64), None, 16)
    assert len(k0) == 0 and na0 == 0 and nm0 == 0 and (m0 == -1).all()
    rig.lm.kf_put(0x850, np.zeros(40, np.uint64))
    k0, q0, na0, nm0, m0 = rig.lm.search_loop_points(_target_record(T), len(T["kps"]), np.array([0x850], np.uint64), None, 16)
    assert len(k0) == 0 and na0 == 0 and nm0 == 0 and (m0 == -1).all()
    rig.close()


def test_claim_scene(oracle):
    sc = S.claim_scene()
    rig = Rig(sc)
    ix = sc["ix"]
    keys, code, nm, match = rig.loop_points(oracle, sc["targets"][0], sc["loop_rows"], sc["matched"])
    assert nm == 4 and match.tolist() == [ix["first"], ix["second"], -1, ix["closed_best"], ix["tie_a"]]
    rig.sim3(oracle, [0])
    rig.close()


def test_errors_leave_the_outputs_alone(oracle):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    from orbhip.extractor import ORBextractor, ORBmatcher
    sc = S.edge_scene()
    rig = Rig(sc, max_kfs=8, max_row=8192)
    T = sc["targets"][0]
    L, h = rig.ex._L, rig.ex.handle
    n, nf = len(sc["loop"]), len(T["kps"])
    kps, desc = sc["sets"][S.SET_A]
    rig.m.put_set(0x501, kps, desc)                                      # no grid
    for k in range(4):
        rig.m.put_set(0x510 + k, kps, desc, None, T["gp"])               # with SET_A: five distinct sets
    rng = np.random.default_rng(1)
    big = np.zeros(1 << 20, capi.KP_DTYPE)                               # one feature too many for the 20-bit position
    big["x"], big["y"] = rng.uniform(1, S.W - 1, len(big)).astype(f32), rng.uniform(1, S.H - 1, len(big)).astype(f32)
    rig.m.put_set(0x503, big, np.zeros((len(big), 32), np.uint8), None, T["gp"])
    rig.lm.kf_put(0x602, np.zeros(8192, np.uint64))
    rig.lm.kf_put(0x603, sc["keys"][:10])

    def sim3(recs=None, K=None, rows=(S.ROWS[0],), keys=None, nn=None, **kw):
        recs = _target_record(T, **kw) if recs is None else recs
        K = len(recs) if K is None else K
        keys = sc["loop"] if keys is None else keys
        nn = len(keys) if nn is None else nn
        rk = np.resize(np.array(rows, np.uint64), max(K, 1))
        q, bi, bd = np.full(n * 32, 0x5A, np.uint8), np.full(n, 0x5A5A5A5A, np.int32), np.full(n, 0x5A5A5A5A, np.int32)
        na = np.full(8, -7, np.int32)
        rc = L.orbhip_fuse_sim3(h, _p(recs), _p(rk), K, _p(np.ascontiguousarray(keys, np.uint64)), nn, _p(q), _p(bi), _p(bd), _p(na))
        assert (q == 0x5A).all() and (bi == 0x5A5A5A5A).all() and (bd == 0x5A5A5A5A).all() and (na == -7).all()
        return rc

    def loop(kf_keys=(0x603,), rec=None, cap=None, **kw):
        rec = _target_record(T, **kw) if rec is None else rec
        kk = np.array(kf_keys, np.uint64)
        keys, q = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(n * 32, 0x5A, np.uint8)
        match = np.full(nf, 0x5A5A5A5A, np.int32)
        npts, na, nm = C.c_int(-7), C.c_int(-7), C.c_int(-7)
        rc = L.orbhip_search_loop_points(h, _p(rec), len(kk), _p(kk), None, 50, _p(keys), n if cap is None else cap, C.byref(npts), _p(q),
                                         C.byref(na), _p(match), C.byref(nm))
        assert (keys == 0x5A5A5A5A5A5A5A5A).all() and (q == 0x5A).all() and (match == 0x5A5A5A5A).all()
        assert npts.value == -7 and na.value == -7 and nm.value == -7
        return rc

    def with_key(key):
        r = _target_record(T)
        r["set_key"] = key
        return r

    assert sim3(rows=(0x999,)) == E_ARG and sim3(recs=with_key(0x999)) == E_ARG and sim3(recs=with_key(0x501)) == E_ARG
    assert sim3(K=-1) == E_ARG and sim3(nn=-1) == E_ARG
    assert sim3(nlevels=0) == E_ARG and sim3(nlevels=17) == E_ARG and sim3(th=np.inf) == E_ARG and sim3(th=np.nan) == E_ARG
    twice = sc["loop"].copy()
    twice[5] = twice[2]
    assert sim3(keys=twice) == E_ARG                                     # a key twice in point_keys
    assert rig.m.set_limit(4) == 4
    five = np.concatenate([with_key(k) for k in (S.SET_A, 0x510, 0x511, 0x512, 0x513)])
    assert sim3(recs=five) == E_ARG                                      # more distinct keys than the limit in force
    assert rig.m.set_limit(96) == 96
    assert sim3(recs=with_key(0x503)) == E_SIZE
    assert sim3(recs=np.repeat(_target_record(T), 65536)) == E_SIZE      # more targets than one launch takes
    many = (np.arange(8192, dtype=np.uint64) + np.uint64(1)) * np.uint64(3)
    assert sim3(recs=np.repeat(_target_record(T), 2049), keys=many) == E_SIZE   # K * n = 2049 * 8192: just beyond 2^24
    assert sim3(K=0) == 0                                                # OK, and nothing is written
    q0, bi0, bd0, na0 = rig.lm.fuse_sim3(_target_record(T), [S.ROWS[0]], sc["loop"][:0])
    assert bi0.shape == (1, 0) and na0.tolist() == [0]                   # n == 0: the counts are zero, nothing is launched
    assert loop(kf_keys=(0x603, 0x999)) == E_ARG
    assert loop(rec=with_key(0x999)) == E_ARG and loop(rec=with_key(0x501)) == E_ARG
    assert loop(nlevels=0) == E_ARG and loop(nlevels=17) == E_ARG and loop(th=np.inf) == E_ARG
    assert loop(rec=with_key(0x503)) == E_SIZE
    assert loop(kf_keys=(0x602,) * 2049) == E_SIZE                       # 2049 * 8192 row entries: beyond 2^24
    assert loop(cap=-1) == E_ARG
    # nothing was left behind: the calls still give the model's answer
    rig.sim3(oracle, [0])
    rig.close()
    # no store; a store without a key-frame table
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    mm = ORBmatcher(0.8, True, ctx=ex)
    mm.put_set(S.SET_A, kps, desc, None, T["gp"])
    h = ex.handle
    assert sim3() == E_ARG and loop() == E_ARG
    lm = localmap.LocalMap(ex, 64)
    assert sim3() == E_ARG and loop() == E_ARG                           # a non-zero row key, and no table
    q, bi, bd, na = lm.fuse_sim3(_target_record(T), None, sc["loop"])    # without row keys a store is enough
    assert not na.any() and (bi == -1).all()                             # (it holds no points)
    mm.close()
    ex.close()


def _table_state(lm, kf_keys, probe):
    return [lm.collect(np.array([k], np.uint64), 1024).tobytes() for k in kf_keys] + [a.tobytes() for a in lm.vote(probe)]


def test_kf_set_batch_equals_the_per_key_frame_calls():
    """Two contexts with the same store and table: one takes orbhip_map_kf_set per key frame, the other the batch.  Entries of 1, 2
    and 33 key frames in one call; every refused input leaves the table as it was."""
    from orbhip import capi, localmap
    from orbhip.extractor import ORBextractor
    rng = np.random.default_rng(3)
    npts, nkf, rowlen = 400, 40, 48
    keys = (np.arange(npts, dtype=np.uint64) + np.uint64(1)) * np.uint64(7919)
    pos = rng.standard_normal((npts, 3)).astype(f32)
    a = [pos, pos, np.ones(npts, f32), np.full(npts, 2, f32), rng.integers(0, 256, (npts, 32), dtype=np.uint8), np.ones(npts, np.uint8)]
    kf_keys = np.arange(nkf, dtype=np.uint64) + np.uint64(0x900)
    rows = {int(k): np.where(rng.random(rowlen) < 0.5, keys[rng.permutation(npts)[:rowlen]], 0).astype(np.uint64) for k in kf_keys}
    ctx, lms = [], []
    for _ in range(2):
        ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        lm = localmap.LocalMap(ex, 512, 64, 64)
        lm.put(keys, *a)
        for k, r in rows.items():
            lm.kf_put(k, r)
        ctx.append(ex)
        lms.append(lm)
    one, batch = lms
    probe = keys[::2]
    mirror = {k: r.copy() for k, r in rows.items()}

    def edits(which, per):
        """`per` edits in each key frame of `which`, interleaved across the key frames: a free point in, NULL in, or a move."""
        out = []
        for kf in which:
            r = mirror[int(kf)]
            free = [k for k in keys[rng.permutation(npts)] if k not in set(r.tolist())][:per]
            for j, idx in enumerate(rng.permutation(rowlen)[:per]):
                val = np.uint64(0) if j % 3 == 2 else free[j]
                r[idx] = val
                out.append((int(kf), int(idx), int(val)))
        return [out[i] for i in rng.permutation(len(out))]

    for which, per in ((kf_keys[:1], 5), (kf_keys[3:5], 7), (kf_keys[5:38], 4), (kf_keys[:33], 1)):
        e = edits(which, per)
        kk, idx, val = (np.array([x[c] for x in e], t) for c, t in ((0, np.uint64), (1, np.int32), (2, np.uint64)))
        batch.kf_set_batch(kk, idx, val)
        for kf in dict.fromkeys(kk.tolist()):                              # the per-key-frame calls, in the same order
            m = kk == np.uint64(kf)
            one.kf_set(kf, idx[m], val[m])
        assert _table_state(one, kf_keys, probe) == _table_state(batch, kf_keys, probe)
        for kf in which:
            want = np.array([k for k in mirror[int(kf)] if k], np.uint64)
            assert np.array_equal(batch.collect(np.array([kf], np.uint64), 1024), want)
    # refused inputs: the table stays as it was
    state = _table_state(batch, kf_keys, probe)
    r0 = mirror[int(kf_keys[0])]
    held = int(r0[r0 != 0][0])
    at_held = int(np.nonzero(r0 == held)[0][0])
    other = (at_held + 1) % rowlen
    absent = int([k for k in keys if k not in set(r0.tolist())][0])
    ok = (int(kf_keys[1]), 0, 0)
    for bad in ([(0x9999, 0, 0)], [(int(kf_keys[0]), rowlen, absent)], [(int(kf_keys[0]), -1, absent)], [(int(kf_keys[0]), 0, 123456789)],
                [(int(kf_keys[0]), other, held)], [(int(kf_keys[0]), 3, absent), (int(kf_keys[0]), 3, 0)], [(0, 0, 0)]):
        e = [ok] + bad
        kk, idx, val = (np.array([x[c] for x in e], t) for c, t in ((0, np.uint64), (1, np.int32), (2, np.uint64)))
        with pytest.raises(capi.OrbHipError):
            batch.kf_set_batch(kk, idx, val)
        assert _table_state(batch, kf_keys, probe) == state
    # a point moves inside one row in one call: the index it leaves is emptied by a later entry of the same call
    batch.kf_set_batch([kf_keys[0], kf_keys[0]], [other, at_held], [held, 0])
    one.kf_set(int(kf_keys[0]), [other, at_held], [held, 0])
    assert _table_state(one, kf_keys, probe) == _table_state(batch, kf_keys, probe)
    batch.kf_set_batch(np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint64))      # m == 0
    for ex in ctx:
        ex.close()
