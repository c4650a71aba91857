"""orbhip_fuse_row / orbhip_fuse_collect on the device against the independent model (tests/fuse_model.py) by bit pattern -- queries
as 32-byte records, best_idx, best_dist, n_active -- and against the path that existed before them: the model's queries and the
points' descriptors uploaded to orbhip_window_best_set, which runs none of the new kernels.  tests/test_fuse_model.py shows on the
CPU that the scenes contain what these tests rely on."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as FM
import fuse_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE, E_CAPACITY = -1, -2, -3


def _target_record(T, **kw):
    from orbhip import localmap
    cam = T["cam"]
    rec = localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                          cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], T["th"])
    for k, v in kw.items():
        rec[k] = v
    return localmap.fuse_target(T["key"], rec, T["sig"])


class Rig:
    """One context: the scene's target sets (with a grid), its points in the store and in the model's store, the source key frame's
    row in the key-frame table; the scene's stale points are erased after the row was put."""

    def __init__(self, sc, max_points=2048, max_kfs=32, max_row=1024, rows=None):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.sc = sc
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.m = ORBmatcher(0.8, True, ctx=self.ex)
        for key, (kps, desc) in sc["sets"].items():
            self.m.put_set(key, kps, desc, None, sc["targets"][0]["gp"])
        self.lm = localmap.LocalMap(self.ex, max_points, max_kfs, max_row)
        self.lm.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
        self.lm.kf_put(S.SRC_ROW, sc["row"])
        for key, r in (rows or {}).items():           # (a row can only be put while the store knows its points)
            self.lm.kf_put(key, r)
        self.lm.erase(sc["keys"][sc["stale"]])
        self.model = S.model_store(sc)

    def records(self, which):
        return np.concatenate([_target_record(self.sc["targets"][k]) for k in which])

    def u_right(self, which, mono=False):
        """The targets' mvuRight one after the other (all -1 for a monocular one); None when none of them has any."""
        T = [self.sc["targets"][k] for k in which]
        if mono or all(t["u_right"] is None for t in T):
            return None
        return np.concatenate([np.full(len(t["kps"]), -1, f32) if t["u_right"] is None else t["u_right"] for t in T])

    def check_target(self, oracle, T, keys, skip, gq, gbi, gbd, gna, mono=False):
        from orbhip import guided
        T = dict(T, u_right=None) if mono else T
        q, code, qd, na, bi, bd = FM.fuse(oracle, self.model, T, T["th"], keys, skip)
        if gq is not None:
            assert gq.tobytes() == q.tobytes(), np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(gq, q)])[0]
        assert gna == na and np.array_equal(gbi, bi) and np.array_equal(gbd, bd)
        obi, obd = guided.WindowBestSet(self.ex, T["key"], q, qd, T["u_right"], T["sig"])     # the old path
        assert np.array_equal(obi, gbi) and np.array_equal(obd, gbd)
        return q, code, bi, bd

    def row(self, oracle, which, n=None, row_key=S.SRC_ROW, skip=True, mono=False, want_queries=True):
        sc = self.sc
        n = len(sc["row"]) if n is None else n
        sk = np.ascontiguousarray(sc["skip"][list(which), :n]) if skip else None
        gq, gbi, gbd, gna = self.lm.fuse_row(row_key, n, self.records(which), sk, self.u_right(which, mono), want_queries)
        out = []
        for j, k in enumerate(which):
            out.append(self.check_target(oracle, sc["targets"][k], sc["row"][:n], None if sk is None else sk[j],
                                         None if gq is None else gq[j], gbi[j], gbd[j], gna[j], mono))
        return out

    def close(self):
        self.m.close()
        self.ex.close()


@pytest.fixture(scope="module")
def main_scene(oracle):
    return S.make(oracle)


def test_main_scene_bit_for_bit(oracle, main_scene):
    rig = Rig(main_scene)
    out = rig.row(oracle, range(5))                   # five records over four sets, one key twice, stereo and monocular together
    assert sum(int((o[3] <= FM.TH_LOW).sum()) for o in out) >= 250 and all((o[1] == FM.ACTIVE).sum() >= 100 for o in out)
    rig.row(oracle, [1])                              # K = 1, a monocular target: u_right NULL
    rig.row(oracle, [0, 1])                           # K = 2: a stereo and a monocular target in one call
    rig.row(oracle, [0, 4], mono=True)                # stereo sets searched as monocular ones: the 5.99 gate everywhere
    rig.row(oracle, [3, 2, 0], skip=False)            # skip NULL
    rig.row(oracle, range(5), want_queries=False)     # the queries stay on the device
    rig.close()


def test_row_lengths_at_wave_and_block_edges(oracle, main_scene):
    """1, 63, 64, 65, 255, 256, 257 entries: the ballot count of one wave, of a block and of the block after it; the last 16-lane
    row of the search; K = 1, 2 and 5."""
    sc = main_scene
    rig = Rig(sc, rows={0x800 + i: sc["row"][:n] for i, n in enumerate(S.SIZES)})
    active = 0
    for i, n in enumerate(S.SIZES):
        for which in ([2], [0, 1], range(5)):
            out = rig.row(oracle, which, n=n, row_key=0x800 + i)
            active += sum(int((o[1] == FM.ACTIVE).sum()) for o in out)
    assert active > 2000
    rig.close()


def test_edge_scene(oracle):
    sc = S.edge_scene()
    rig = Rig(sc)
    (q, code, bi, bd), = rig.row(oracle, [0])
    ix = sc["ix"]
    for case, want in S.EDGE_EXPECT.items():
        assert (code[ix[case]] != FM.ACTIVE) if want is None else (code[ix[case]] == want), case
    assert bi[ix["gate_mono_on"]] >= 0 and bi[ix["gate_mono_out"]] == -1 and bi[ix["gate_stereo_on"]] >= 0 and bi[ix["gate_stereo_out"]] == -1
    rig.row(oracle, [0], skip=False)                  # the skipped entry takes part now
    # the erased point's slot goes to another point: the row's entry still resolves to nothing
    k = ix["stale"]
    old = sc["keys"][k]
    fresh = np.array([999331], np.uint64)
    a = [sc[name][[k]] for name in ("pos", "normal", "min_dist", "max_dist", "pdesc", "flags")]
    rig.lm.put(fresh, *a)
    rig.model.put(fresh, *a)
    assert old != fresh[0] and int(old) not in rig.model.pts
    (q2, code2, _, _), = rig.row(oracle, [0])
    assert code2[k] == FM.UNKNOWN and np.array_equal(code2, code)
    rig.close()


def test_association_of_u_decides_a_bound(oracle):
    sc, ua, ub = S.assoc_scene()
    rig = Rig(sc)
    (q, code, bi, bd), = rig.row(oracle, [0])
    assert (code[0] == FM.ACTIVE) == (ua < ub)         # with (fx * xc) * invz the point would land on the other side of mnMaxX
    rig.close()


def _collect_rows(sc):
    """Three candidate rows over the scene's points (two of them overlap) and the target's own row: some of the candidates, empty
    entries.  All of them hold entries that are stale by the time of the call."""
    row = sc["row"]
    rows = {0x900: row[:200], 0x901: row[100:350][::-1].copy(), 0x902: row[300:]}
    own = np.concatenate([row[5:400:7], np.zeros(9, np.uint64)])
    return rows, own


def _collect_check(oracle, rig, T, rows, own, cap=1024, mono=False):
    kf_keys = np.array(list(rows), np.uint64)
    keys, gq, gbi, gbd, gna = rig.lm.fuse_collect(_target_record(T), S.CUR_ROW, kf_keys, cap, None if mono else T["u_right"])
    assert np.array_equal(keys, rig.lm.collect(kf_keys, cap))
    assert np.array_equal(keys, FM.collect(rig.model, list(rows.values())))
    held = {int(k) for k in own if int(k) in rig.model.pts}
    skip = np.array([int(k) in held for k in keys], np.uint8)
    q, code, bi, bd = rig.check_target(oracle, T, keys, skip, gq, gbi, gbd, gna, mono)
    assert (code[skip.astype(bool)] == FM.SKIPPED).all() or not skip.any()
    assert not gq[skip.astype(bool)].tobytes().strip(b"\0")          # IsInKeyFrame: inactive, all zero
    return keys, code, skip, bi, bd


def test_collect_second_pass(oracle, main_scene):
    sc = main_scene
    rows, own = _collect_rows(sc)
    rig = Rig(sc, rows={**rows, S.CUR_ROW: own})
    T = sc["targets"][0]
    assert any(int(k) and int(k) not in rig.model.pts for k in own)      # a stale entry in the target's own row
    frame_keys = sc["row"][::3]
    before = rig.lm.vote(frame_keys)
    keys, code, skip, bi, bd = _collect_check(oracle, rig, T, rows, own)
    assert skip.sum() >= 30 and (code == FM.ACTIVE).sum() >= 100 and (bd <= FM.TH_LOW).sum() >= 50
    _collect_check(oracle, rig, T, rows, own, mono=True)
    after = rig.lm.vote(frame_keys)                    # the marks are clear again
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[1].sum() > 100
    # points leave the map, among them some the target holds and some that were candidates; their slots go to new points, which
    # enter a candidate row: the stale entries of the target's own row must not mark them
    gone_own = np.array([k for k in own if int(k) in rig.model.pts][:12], np.uint64)
    gone = np.concatenate([gone_own, keys[(code == FM.ACTIVE) & ~skip.astype(bool)][:20]])
    old_slots = rig.lm.slots(gone)
    rig.lm.erase(gone)
    rig.model.erase(gone)
    fresh = (np.arange(len(gone), dtype=np.uint64) + np.uint64(1)) * np.uint64(1000003)
    at = [int(np.nonzero(sc["keys"] == k)[0][0]) for k in gone]
    a = [sc[name][at] for name in ("pos", "normal", "min_dist", "max_dist", "pdesc", "flags")]
    a[5] = np.ones(len(gone), np.uint8)
    rig.lm.put(fresh, *a)
    rig.model.put(fresh, *a)
    assert set(rig.lm.slots(fresh)) == set(old_slots)
    rows[0x903] = fresh
    rig.lm.kf_put(0x903, fresh)
    keys2, code2, skip2, _, _ = _collect_check(oracle, rig, T, rows, own)
    pos = {int(k): i for i, k in enumerate(keys2)}
    assert all(int(k) in pos and not skip2[pos[int(k)]] for k in fresh) and not set(gone.tolist()) & set(pos)
    assert (code2[[pos[int(k)] for k in fresh[:12]]] != FM.SKIPPED).all()
    # too little room: the first cap keys, the number, nothing else
    from orbhip import capi
    with pytest.raises(capi.OrbHipError) as e:
        rig.lm.fuse_collect(_target_record(T), S.CUR_ROW, np.array(list(rows), np.uint64), 100, T["u_right"])
    assert e.value.total == len(keys2) and np.array_equal(e.value.partial, keys2[:100])
    # an empty list of key frames, and rows that hold nothing
    k0, q0, bi0, bd0, na0 = rig.lm.fuse_collect(_target_record(T), S.CUR_ROW, np.zeros(0, np.uint64), 16, T["u_right"])
    assert len(k0) == 0 and na0 == 0
    rig.lm.kf_put(0x904, np.zeros(40, np.uint64))
    k0, q0, bi0, bd0, na0 = rig.lm.fuse_collect(_target_record(T), S.CUR_ROW, np.array([0x904], np.uint64), 16, T["u_right"])
    assert len(k0) == 0 and na0 == 0
    rig.close()


def test_errors_leave_the_outputs_alone(oracle):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    from orbhip.extractor import ORBextractor, ORBmatcher
    sc = S.edge_scene()
    rig = Rig(sc, max_kfs=8, max_row=8192)
    T = sc["targets"][0]
    L, h = rig.ex._L, rig.ex.handle
    n = len(sc["row"])
    kps, desc = sc["sets"][S.SET_A]
    rig.m.put_set(0x501, kps, desc)                                      # no grid
    for k in range(4):
        rig.m.put_set(0x510 + k, kps, desc, None, T["gp"])               # with SET_A: five distinct sets
    rng = np.random.default_rng(1)
    big = np.zeros(1 << 20, capi.KP_DTYPE)                               # one feature too many for the 20-bit position
    big["x"], big["y"] = rng.uniform(1, S.W - 1, len(big)).astype(f32), rng.uniform(1, S.H - 1, len(big)).astype(f32)
    rig.m.put_set(0x503, big, np.zeros((len(big), 32), np.uint8), None, T["gp"])
    rig.lm.kf_put(S.CUR_ROW, sc["row"][:10])
    rig.lm.kf_put(0x602, np.zeros(8192, np.uint64))
    ur = T["u_right"]

    def row(src=S.SRC_ROW, recs=None, K=None, **kw):
        recs = _target_record(T, **kw) if recs is None else recs
        K = len(recs) if K is None else K
        q, bi, bd = np.full(n * 32, 0x5A, np.uint8), np.full(n, 0x5A5A5A5A, np.int32), np.full(n, 0x5A5A5A5A, np.int32)
        na = np.full(8, -7, np.int32)
        rc = L.orbhip_fuse_row(h, src, _p(recs), K, None, _p(ur), _p(q), _p(bi), _p(bd), _p(na))
        assert (q == 0x5A).all() and (bi == 0x5A5A5A5A).all() and (bd == 0x5A5A5A5A).all() and (na == -7).all()
        return rc

    def collect(cur=S.CUR_ROW, kf_keys=(S.SRC_ROW,), rec=None, **kw):
        rec = _target_record(T, **kw) if rec is None else rec
        kk = np.array(kf_keys, np.uint64)
        keys, q = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(n * 32, 0x5A, np.uint8)
        bi, bd = np.full(n, 0x5A5A5A5A, np.int32), np.full(n, 0x5A5A5A5A, np.int32)
        nc, na = C.c_int(-7), C.c_int(-7)
        rc = L.orbhip_fuse_collect(h, _p(rec), cur, len(kk), _p(kk), _p(ur), _p(keys), n, C.byref(nc), _p(q), _p(bi), _p(bd), C.byref(na))
        assert (keys == 0x5A5A5A5A5A5A5A5A).all() and (q == 0x5A).all() and (bi == 0x5A5A5A5A).all() and (bd == 0x5A5A5A5A).all()
        assert nc.value == -7 and na.value == -7
        return rc

    def with_key(key):
        r = _target_record(T)
        r["set_key"] = key
        return r

    assert row(src=0x999) == E_ARG and row(recs=with_key(0x999)) == E_ARG and row(recs=with_key(0x501)) == E_ARG
    assert row(K=-1) == E_ARG
    assert row(nlevels=0) == E_ARG and row(nlevels=17) == E_ARG and row(th=np.inf) == E_ARG and row(th=np.nan) == E_ARG
    assert rig.m.set_limit(4) == 4
    five = np.concatenate([with_key(k) for k in (S.SET_A, 0x510, 0x511, 0x512, 0x513)])
    assert row(recs=five) == E_ARG                                       # more distinct keys than the limit in force
    assert rig.m.set_limit(96) == 96
    assert row(recs=with_key(0x503)) == E_SIZE
    assert row(src=0x602, recs=np.repeat(_target_record(T), 2049)) == E_SIZE   # K * n = 2049 * 8192: just beyond 2^24
    assert row(recs=np.repeat(_target_record(T), 65536)) == E_SIZE       # more targets than one launch takes
    assert row(K=0) == 0                                                 # OK, and nothing is written
    assert collect(cur=0x999) == E_ARG and collect(kf_keys=(S.SRC_ROW, 0x999)) == E_ARG
    assert collect(rec=with_key(0x999)) == E_ARG and collect(rec=with_key(0x501)) == E_ARG
    assert collect(nlevels=0) == E_ARG and collect(nlevels=17) == E_ARG and collect(th=np.inf) == E_ARG
    assert collect(rec=with_key(0x503)) == E_SIZE
    assert collect(kf_keys=(0x602,) * 2049) == E_SIZE                    # 2049 * 8192 row entries: beyond 2^24
    # nothing was left behind: the calls still give the model's answer
    rig.row(oracle, [0])
    rig.close()
    # no store; a store without a key-frame table
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    mm = ORBmatcher(0.8, True, ctx=ex)
    mm.put_set(S.SET_A, kps, desc, None, T["gp"])
    h = ex.handle
    assert row() == E_ARG and collect() == E_ARG
    localmap.LocalMap(ex, 64)
    assert row() == E_ARG and collect() == E_ARG
    mm.close()
    ex.close()
