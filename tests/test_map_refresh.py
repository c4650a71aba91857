"""orbhip_map_refresh / orbhip_map_get on the device, through the Python mirror, against the independent numpy model
(tests/refresh_model.py): every output and the store itself bit for bit, floats by bit pattern.  tests/test_refresh_model.py shows on
the CPU that the guard scene contains what these tests rely on."""
import numpy as np
import pytest

import refresh_model as R

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE = -1, -2
LENGTHS = [1, 2, 3, 15, 16, 17, 32, 33, 40]       # the 16-lane round edges


@pytest.fixture(scope="module")
def ctx():
    from orbhip.extractor import ORBextractor, ORBmatcher
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    m = ORBmatcher(0.8, True, ctx=ex)
    yield ex, m
    m.close()
    ex.close()


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class Rig:
    """The scene's sets and points resident in one context, and the model's copy of the store."""

    def __init__(self, ctx, sc, max_points=512):
        from orbhip import localmap
        self.ex, self.m = ctx
        self.sc = sc
        self.m.drop_set(0)
        assert self.m.set_limit(96) == 96
        for k, (kps, desc) in enumerate(sc["sets"]):
            self.m.put_set(int(sc["set_keys"][k]), kps, desc)
        self.lm = localmap.LocalMap(self.ex, max_points)          # (a new store: the last rig's is dropped)
        self.store = {k: np.array(sc[k]).copy() for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags")}
        self.lm.put(sc["keys"], *[self.store[k] for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags")])
        self.kfs = np.zeros(len(sc["sets"]), localmap.REFRESH_KF_DTYPE)
        self.kfs["set_key"], self.kfs["Ow"], self.kfs["flags"] = sc["set_keys"], sc["Ow"], sc["kf_flags"]

    def get(self, which=None):
        keys = self.sc["keys"] if which is None else self.sc["keys"][which]
        return self.lm.map_get(keys)

    def check_store(self):
        g = self.get()
        for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags"):
            assert same(g[k], self.store[k]), k

    def refresh(self, what, P=None, nlevels=None):
        """The first P points of the scene through the call, compared with the model on the store as it stands; returns the status."""
        sc = self.sc
        P = len(sc["keys"]) if P is None else P
        sub = dict(sc, keys=sc["keys"][:P], off=sc["off"][:P + 1], ref_pos=sc["ref_pos"][:P], nlevels=nlevels or sc["nlevels"])
        st = {k: v[:P] for k, v in self.store.items()}
        want = R.refresh(sub, what, st)
        n = sub["off"][P]
        got = self.lm.map_refresh(sc["sf"], sub["nlevels"], what, self.kfs, sub["keys"], sub["off"], sc["obs_kf"][:n], sc["obs_idx"][:n],
                                  sub["ref_pos"])
        for name, g, w in zip(("status", "best_pos", "desc", "normal", "min_dist", "max_dist"), got, want):
            assert same(g, w), (name, np.nonzero([not same(a, b) for a, b in zip(g, w)])[0][:8])
        self.store["desc"][:P], self.store["normal"][:P] = want[2], want[3]
        self.store["min_dist"][:P], self.store["max_dist"][:P] = want[4], want[5]
        self.check_store()                                         # write equals read-back, and nothing else moved
        return want[0]


@pytest.mark.parametrize("what", [1, 2, 3])
def test_list_lengths_at_the_round_edges(ctx, what):
    sc = R.make_scene(21, nkf=40, P=36, lengths=LENGTHS, nfeat=(40, 64), bad_kfs=(5, 17, 33))
    status = Rig(ctx, sc).refresh(what)
    assert ((status & 2) == (what & 2)).all() and ((status & 1) <= (what & 1)).all()
    assert what == 2 or (status & 1).sum() >= 30                   # (a point seen from bad key frames alone keeps its descriptor)


@pytest.mark.parametrize("P", [1, 15, 16, 17, 300])
def test_batch_sizes_at_the_block_edge(ctx, P):
    sc = R.make_scene(22, nkf=20, P=300, nfeat=(48, 64), bad_kfs=(3,))
    rig = Rig(ctx, sc)
    assert ((rig.refresh(3, P) & 2) == 2).all()
    assert ((rig.refresh(1, P) & 2) == 0).all() and (rig.refresh(2, P) == 2).all()   # on the refreshed store: the same values again


def test_guard_scene(ctx):
    sc = R.guard_scene()
    cnt = R.guard_counts(sc)
    assert all(cnt[k] >= 1 for k in "abcdefg"), cnt
    Rig(ctx, sc).refresh(3)


@pytest.mark.parametrize("ref", ["first", "last", "bad"])
def test_reference_observer_position(ctx, ref):
    sc = R.make_scene(23, nkf=10, P=60, bad_kfs=(4,), ref="first" if ref == "bad" else ref)
    if ref == "bad":
        hit = 0
        for p in range(60):
            a, b = sc["off"][p], sc["off"][p + 1]
            w = np.nonzero(sc["obs_kf"][a:b] == 4)[0]
            if len(w):
                sc["ref_pos"][p], hit = w[0], hit + 1
        assert hit >= 5
    Rig(ctx, sc).refresh(3)


@pytest.mark.parametrize("nlevels", [1, 8, 16])
def test_octaves_at_both_ends(ctx, nlevels):
    for octave in sorted({0, nlevels - 1}):
        sc = R.make_scene(24 + octave, nkf=6, P=20, nlevels=nlevels, octave=octave)
        rig = Rig(ctx, sc)
        rig.refresh(2)
        want = (rig.store["max_dist"] / sc["sf"][nlevels - 1]).astype(f32)
        assert same(rig.store["min_dist"], want)


def test_points_left_alone(ctx):
    sc = R.make_scene(25, nkf=8, P=40, lengths=[4, 2, 0, 5, 1], bad_points=(6, 18))
    rig = Rig(ctx, sc)
    alone = [p for p in range(40) if p % 5 == 2 or p in (6, 18)]
    before = rig.get(alone)
    status = rig.refresh(3)
    after = rig.get(alone)
    assert (status[alone] == 0).all() and (np.delete(status, alone) == 3).all()
    assert all(same(before[k], after[k]) for k in before)


def test_all_observers_bad(ctx):
    sc = R.make_scene(26, nkf=5, P=20, bad_kfs=range(5))
    rig = Rig(ctx, sc)
    status = rig.refresh(3)
    assert (status == 2).all() and same(rig.store["desc"], sc["desc"])
    assert not same(rig.store["normal"], sc["normal"])
    assert (Rig(ctx, sc).refresh(1) == 0).all()


def test_null_outputs(ctx):
    sc = R.make_scene(27, nkf=8, P=33)
    rig = Rig(ctx, sc)
    want = R.refresh(sc, 3, rig.store)
    got = rig.lm.map_refresh(sc["sf"], sc["nlevels"], 3, rig.kfs, sc["keys"], sc["off"], sc["obs_kf"], sc["obs_idx"], sc["ref_pos"], want=False)
    assert same(got[0], want[0]) and all(g is None for g in got[1:])
    g = rig.get()
    assert same(g["desc"], want[2]) and same(g["normal"], want[3]) and same(g["min_dist"], want[4]) and same(g["max_dist"], want[5])


def test_search_after_refresh_equals_search_after_put(ctx):
    """orbhip_search_local_points over the refreshed store and over a second store that orbhip_map_put filled with the model's values."""
    from orbhip import localmap
    sc = R.make_scene(28, nkf=12, P=200, nfeat=(48, 64))
    sc["Ow"] = (sc["Ow"] * f32(0.2)).astype(f32)                   # observers near the frame's camera: the points are seen from the front
    rig = Rig(ctx, sc)
    rig.refresh(3)
    rng = np.random.RandomState(5)
    n, FRAME = 400, 0x7000
    kps = np.zeros(n, R.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"], kps["size"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.randint(0, 8, n), 31
    fdesc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    fdesc[:200] = rig.store["desc"]
    pos = sc["pos"]
    kps["x"][:200] = np.clip(300 * pos[:, 0] / pos[:, 2] + 320, 1, 638)
    kps["y"][:200] = np.clip(300 * pos[:, 1] / pos[:, 2] + 240, 1, 478)
    rig.m.put_set(FRAME, kps, fdesc, None, (0.0, 0.0, 64 / 640.0, 48 / 480.0))
    cam = localmap.camera(np.eye(3), np.zeros(3), np.zeros(3), 300, 300, 320, 240, 0, (0, 640, 0, 480), sc["sf"][:8], np.log(f32(1.2)), 0.5, 3.0)
    skip = np.zeros(200, np.uint8)
    a = rig.lm.search(FRAME, n, cam, sc["keys"], skip)
    assert a[1] >= 20                                               # points in view: the refreshed normals and ranges are read
    second = localmap.LocalMap(rig.ex, 512)
    second.put(sc["keys"], *[rig.store[k] for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags")])
    b = second.search(FRAME, n, cam, sc["keys"], skip)
    assert same(a[0], b[0]) and a[1:3] == b[1:3] and same(a[3], b[3])


def test_flags_generation_and_rows_untouched(ctx):
    from orbhip import localmap
    sc = R.make_scene(29, nkf=8, P=50)
    rig = Rig(ctx, sc)
    again = sc["keys"][10:20]
    rig.lm.erase(again)                                             # their slots' generations move on
    sl = slice(10, 20)
    rig.lm.put(again, *[rig.store[k][sl] for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags")])
    rig.lm.kf_init(4, 64)
    rig.lm.kf_put(0x900, sc["keys"][:30])
    rig.lm.kf_put(0x901, sc["keys"][25:])
    before = rig.lm.collect([0x900, 0x901], 64)
    assert len(before) == 50
    rig.refresh(3)
    assert same(rig.lm.collect([0x900, 0x901], 64), before)
    assert same(rig.get()["flags"], sc["flags"])


def test_map_get(ctx):
    from orbhip import capi
    sc = R.make_scene(30, nkf=4, P=70, bad_points=(3, 9))
    rig = Rig(ctx, sc)
    rig.check_store()
    order = np.random.RandomState(1).permutation(70)[:40]
    g = rig.lm.map_get(sc["keys"][order])
    assert all(same(g[k], rig.store[k][order]) for k in g)
    g = rig.lm.map_get(sc["keys"], want=("normal", "flags"))        # the other outputs NULL
    assert sorted(g) == ["flags", "normal"] and same(g["normal"], rig.store["normal"]) and same(g["flags"], sc["flags"])
    assert rig.lm.map_get(np.zeros(0, np.uint64))["pos"].shape == (0, 3)
    with pytest.raises(capi.OrbHipError):
        rig.lm.map_get([sc["keys"][0], 0x123456])
    with pytest.raises(capi.OrbHipError):
        rig.lm.map_get([0])


def test_errors_change_nothing(ctx):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    sc = R.make_scene(31, nkf=6, P=12, lengths=[3, 2, 4])
    sc["sets"][5][0]["octave"][0] = 7                               # the largest octave of set 5
    rig = Rig(ctx, sc)
    L, h = capi.load(), rig.ex.handle
    P = 12

    def call(what=3, nlevels=8, kfs=None, keys=None, off=None, obs_kf=None, obs_idx=None, ref_pos=None, P=P):
        prm = np.zeros(1, localmap.REFRESH_PARAMS_DTYPE)
        prm["scale_factors"][0], prm["nlevels"], prm["what"] = sc["sf"], nlevels, what
        kfs = rig.kfs if kfs is None else kfs
        a = [np.ascontiguousarray(x, t) for x, t in ((sc["keys"] if keys is None else keys, np.uint64), (sc["off"] if off is None else off, np.int32),
                                                      (sc["obs_kf"] if obs_kf is None else obs_kf, np.int32),
                                                      (sc["obs_idx"] if obs_idx is None else obs_idx, np.int32),
                                                      (sc["ref_pos"] if ref_pos is None else ref_pos, np.int32))]
        m = max(P, 1)
        status = np.full(m, 0x5A, np.uint8)
        outs = [np.full(m, 0x5A5A5A5A, np.int32), np.full((m, 32), 0x5A, np.uint8), np.full((m, 3), 7, f32), np.full(m, 7, f32), np.full(m, 7, f32)]
        rc = L.orbhip_map_refresh(h, _p(prm), len(kfs), _p(kfs), P, *[_p(x) for x in a], _p(status), *[_p(x) for x in outs])
        if rc != 0:                                                 # a failed call changes nothing: neither the outputs nor the store
            assert (status == 0x5A).all() and (outs[0] == 0x5A5A5A5A).all() and (outs[1] == 0x5A).all() and all((o == 7).all() for o in outs[2:])
            rig.check_store()
        return rc

    def edit(name, at, value):
        a = sc[name].copy()
        a[at] = value
        return a

    def with_key(i, key):
        k = rig.kfs.copy()
        k["set_key"][i] = key
        return k

    assert call(keys=edit("keys", 4, 0x999999)) == E_ARG            # an unknown point key
    assert call(keys=edit("keys", 4, sc["keys"][9])) == E_ARG       # a key twice
    assert call(kfs=with_key(2, 0x6123)) == E_ARG                   # a set that is not resident
    assert call(obs_kf=edit("obs_kf", 5, 6)) == E_ARG and call(obs_kf=edit("obs_kf", 5, -1)) == E_ARG
    n3 = len(sc["sets"][sc["obs_kf"][7]][0])
    assert call(obs_idx=edit("obs_idx", 7, n3)) == E_ARG and call(obs_idx=edit("obs_idx", 7, -1)) == E_ARG
    assert call(ref_pos=edit("ref_pos", 0, 3)) == E_ARG and call(ref_pos=edit("ref_pos", 1, -1)) == E_ARG   # (list 0 has 3 rows)
    assert call(nlevels=7) == E_ARG                                 # set 5 holds octave 7
    assert call(nlevels=0) == E_ARG and call(nlevels=17) == E_ARG
    assert call(off=edit("off", 0, 1)) == E_ARG and call(off=edit("off", 3, sc["off"][2] - 1)) == E_ARG
    assert call(what=0) == E_ARG and call(what=4) == E_ARG
    big = np.zeros(1 << 20, np.int32)
    assert call(P=1, off=[0, 1 << 20], obs_kf=big, obs_idx=big, ref_pos=[0], keys=sc["keys"][:1]) == E_SIZE
    assert rig.m.set_limit(4) == 4
    assert call() == E_ARG                                          # six distinct sets, four allowed
    assert rig.m.set_limit(96) == 96
    for k, (kps, desc) in enumerate(sc["sets"]):                    # (lowering the limit dropped sets)
        rig.m.put_set(int(sc["set_keys"][k]), kps, desc)
    assert call(P=0) == 0
    assert call(what=1, ref_pos=edit("ref_pos", 0, 99)) == 0        # ref_pos is read for ORBHIP_REFRESH_NORMAL only
    rig.store["desc"] = R.refresh(sc, 1, rig.store)[2]
    rig.check_store()
    rig.refresh(3)                                                  # and the call still gives the model's answer
