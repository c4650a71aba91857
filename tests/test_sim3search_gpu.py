"""orbhip_search_by_sim3 on the device.  Queries as 32-byte records, best / dist of both directions, n_active, match12 and nfound are
compared by bit pattern against the independent model (tests/sim3search_model.py) and against the path that existed before the call:
the model's queries and the points' descriptors uploaded to orbhip_window_best_set twice and the agreement formed on the host, which
runs none of the new kernels.  Every call is made twice (byte for byte the same), once more with the optional outputs NULL, and is
followed by an orbhip_map_vote against its model, which shows that marks and scratch were left clean.
tests/test_sim3search_model.py shows on the CPU that the scenes contain what these tests rely on."""
import ctypes as C

import numpy as np
import pytest

import sim3search_model as M
import sim3search_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE = -1, -2


def _record(side, **kw):
    from orbhip import localmap
    cam = side["cam"]
    rec = localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                          cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], 1.0)
    for k, v in kw.items():
        rec[k] = v
    return localmap.fuse_target(side["key"], rec, side["sig"])


class Rig:
    """One context: the scene's two sets (with a grid), its points in the store and the two rows in the key-frame table.  The
    scene's stale points are erased after the rows were put and new points take their slots; its erased points just leave."""

    def __init__(self, sc, max_points=2048, max_kfs=8, max_row=512):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.sc = sc
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.m = ORBmatcher(0.8, True, ctx=self.ex)
        self.lm = localmap.LocalMap(self.ex, max_points, max_kfs, max_row)
        self.lm.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
        for side, row in zip(sc["sides"], sc["rows"]):
            self.m.put_set(side["key"], side["kps"], side["desc"], None, side["gp"])
            self.lm.kf_put(side["row_key"], row)
        if len(sc["stale"]):
            old = self.lm.slots(sc["stale"])
            self.lm.erase(sc["stale"])
            self.lm.put(*S.fresh_points(sc))
            new = self.lm.slots(sc["fresh_keys"])
            assert set(new) == set(old) and (new >= 0).all()            # the rows' stale entries name slots that hold other points now
        if len(sc["erased"]):
            self.lm.erase(sc["erased"])
        self.model = S.model_store(sc)
        self.probe = np.concatenate([sc["keys"][::2], sc["fresh_keys"]])

    def vote_model(self):
        live = {int(k) for k in self.probe if int(k) in self.model.pts and not self.model.pts[int(k)][5] & M.MP_BAD}
        rows = {side["row_key"]: row for side, row in zip(self.sc["sides"], self.sc["rows"])}
        cnt = {rk: sum(1 for k in row if int(k) in live) for rk, row in rows.items()}
        keys = sorted(rk for rk, c in cnt.items() if c)
        return np.array(keys, np.uint64), np.array([cnt[k] for k in keys], np.int32)

    def check_vote(self):
        gk, gc = self.lm.vote(self.probe)
        wk, wc = self.vote_model()
        assert np.array_equal(gk, wk) and np.array_equal(gc, wc)

    def call(self, want, th_high=M.TH_HIGH, taken=True, want_outputs=True):
        sc = self.sc
        sR21, t21, sR12, t12 = want["sim"]
        recs = np.concatenate([_record(s) for s in sc["sides"]])
        rk = [s["row_key"] for s in sc["sides"]]
        return self.lm.search_by_sim3(recs, rk, len(sc["rows"][0]), len(sc["rows"][1]), sR21, t21, sR12, t12, sc["th"], th_high,
                                      sc["taken1"] if taken else None, sc["taken2"] if taken else None, want_outputs)

    def check(self, oracle, th_high=M.TH_HIGH, taken=True):
        from orbhip import guided
        sc = self.sc
        want = S.model(oracle, sc, None, th_high, taken)
        match, nf, na, d0, d1 = self.call(want, th_high, taken)
        for d, (gq, gb, gd) in enumerate((d0, d1)):
            q = want["q"][d]
            assert gq.tobytes() == q.tobytes(), (d, np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(gq, q)])[0])
            assert np.array_equal(gb, want["best"][d]) and np.array_equal(gd, want["dist"][d]), d
            dst = sc["sides"][1 - d]
            ob, od = guided.WindowBestSet(self.ex, dst["key"], q, want["qdesc"][d], None, None)       # the old path: no gate
            assert np.array_equal(ob, gb) and np.array_equal(od, gd), d
        assert np.array_equal(na, want["n_active"]) and match.tobytes() == want["match12"].tobytes() and nf == want["nfound"]
        old_match, old_nf = M.agree(d0[1], d0[2], d1[1], d1[2], th_high)                             # the host agreement of the old path
        assert np.array_equal(old_match, match) and old_nf == nf
        self.check_vote()
        again = self.call(want, th_high, taken)                                                       # byte for byte
        assert again[0].tobytes() == match.tobytes() and again[1] == nf and np.array_equal(again[2], na)
        assert all(a.tobytes() == b.tobytes() for x, y in zip(again[3:], (d0, d1)) for a, b in zip(x, y))
        m2, nf2, na2, _, _ = self.call(want, th_high, taken, want_outputs=False)                     # the optional outputs NULL
        assert m2.tobytes() == match.tobytes() and nf2 == nf and np.array_equal(na2, na)
        self.check_vote()
        return want

    def close(self):
        self.m.close()
        self.ex.close()


def test_edge_scene_bit_for_bit(oracle):
    sc = S.edge_scene()
    rig = Rig(sc)
    want = rig.check(oracle)
    code = want["code"][0]
    for case, exp in S.EDGE_EXPECT.items():
        assert code[sc["ix"][case]] == exp, case
    assert want["n_active"].tolist() == [int((code == M.ACTIVE).sum()), 0]
    rig.close()


def test_assoc_scene(oracle):
    sc, ua, ub = S.assoc_scene()
    rig = Rig(sc)
    want = rig.check(oracle)
    assert want["n_active"][0] == (1 if ua < ub else 0)
    rig.close()


def test_agree_scene(oracle):
    sc = S.agree_scene()
    rig = Rig(sc)
    want = rig.check(oracle)
    assert np.array_equal(want["match12"], sc["expect"]) and want["nfound"] == 5
    rig.check(oracle, th_high=M.TH_LOW)                 # another bound
    rig.check(oracle, taken=False)                      # the taken bytes NULL: the two closed pairs agree now
    rig.close()


@pytest.mark.parametrize("n1,n2", S.SIZES + ((50, 40),))
def test_row_shapes_at_wave_and_block_edges(oracle, n1, n2):
    """Rows of 1, 63, 64, 65, 255, 256 and 257 entries on either side: the ballot count of one wave, of a block and of the block after
    it in the projection and in the agreement; n1 != n2."""
    rig = Rig(S.pair_scene(n1, n2))
    want = rig.check(oracle)
    assert want["nfound"] >= 1
    rig.close()


def test_rows_without_a_point_and_the_same_key_frame_twice(oracle):
    for empty in ((True, False), (False, True), (True, True)):
        rig = Rig(S.pair_scene(50, 40, empty=empty))
        want = rig.check(oracle)
        assert want["nfound"] == 0 and (want["match12"] == -1).all()
        rig.close()
    sc = S.same_scene()
    rig = Rig(sc)
    want = rig.check(oracle)
    assert want["nfound"] == int((sc["rows"][0] != 0).sum()) >= 20
    rig.close()


def test_errors_leave_the_outputs_alone(oracle):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    from orbhip.extractor import ORBextractor, ORBmatcher
    sc = S.pair_scene(50, 40)
    rig = Rig(sc, max_row=64)
    L = rig.ex._L
    ctx = {"h": rig.ex.handle}
    n1, n2 = len(sc["rows"][0]), len(sc["rows"][1])
    s1, s2 = sc["sides"]
    sim = [np.ascontiguousarray(a, f32).ravel() for a in S.model(oracle, sc)["sim"]]
    rig.m.put_set(0x951, s2["kps"], s2["desc"])                          # no grid
    rig.m.put_set(0x952, s2["kps"][:30], s2["desc"][:30], None, s2["gp"])   # not as long as row 2
    rng = np.random.default_rng(1)
    big = np.zeros(1 << 20, capi.KP_DTYPE)                               # one feature too many for the 20-bit position
    big["x"], big["y"] = rng.uniform(1, S.W - 1, len(big)).astype(f32), rng.uniform(1, S.H - 1, len(big)).astype(f32)
    rig.m.put_set(0x953, big, np.zeros((len(big), 32), np.uint8), None, s2["gp"])

    def call(rows=(S.ROW1, S.ROW2), set2=None, th=7.5, side=1, **kw):
        recs = np.concatenate([_record(s1, **(kw if side == 0 else {})), _record(s2, **(kw if side == 1 else {}))])
        if set2 is not None:
            recs["set_key"][1] = set2
        rk = np.array(rows, np.uint64)
        out = [np.full(n1, 0x5A5A5A5A, np.int32), np.full(4, -7, np.int32)]
        out += [a for n in (n1, n2) for a in (np.full(n * 32, 0x5A, np.uint8), np.full(n, 0x5A5A5A5A, np.int32), np.full(n, 0x5A5A5A5A, np.int32))]
        nf = C.c_int(-7)
        rc = L.orbhip_search_by_sim3(ctx["h"], _p(recs), _p(rk), _p(sim[0]), _p(sim[1]), _p(sim[2]), _p(sim[3]), C.c_float(th), 100, None, None,
                                     _p(out[0]), C.byref(nf), _p(out[1]), *[_p(a) for a in out[2:]])
        if rc:
            assert nf.value == -7 and (out[1] == -7).all() and all((a == (0x5A if a.dtype == np.uint8 else 0x5A5A5A5A)).all() for a in out[:1] + out[2:])
        return rc

    assert call() == 0
    assert call(rows=(0x999, S.ROW2)) == E_ARG and call(rows=(S.ROW1, 0x999)) == E_ARG           # an unknown row
    assert call(set2=0x999) == E_ARG and call(set2=0x951) == E_ARG                                # an unknown set, a set without a grid
    assert call(set2=0x952) == E_ARG and call(rows=(S.ROW1, S.ROW1)) == E_ARG                     # row and set of different lengths
    for side in (0, 1):
        assert call(side=side, nlevels=0) == E_ARG and call(side=side, nlevels=17) == E_ARG
    assert call(th=np.inf) == E_ARG and call(th=np.nan) == E_ARG
    assert call(set2=0x953) == E_SIZE
    rig.check(oracle)                                                    # nothing was left behind
    rig.close()
    # no store; a store without a key-frame table
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    mm = ORBmatcher(0.8, True, ctx=ex)
    for s in (s1, s2):
        mm.put_set(s["key"], s["kps"], s["desc"], None, s["gp"])
    ctx["h"] = ex.handle
    assert call() == E_ARG
    lm = localmap.LocalMap(ex, 64)
    assert call() == E_ARG
    del lm
    mm.close()
    ex.close()
