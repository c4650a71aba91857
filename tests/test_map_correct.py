"""orbhip_map_correct_sim3 / orbhip_map_correct_se3 on the device, through the Python mirror, against the independent numpy model
(tests/correct_model.py): every output and the store itself, read back through orbhip_map_get, bit for bit, floats by bit pattern.
tests/test_correct_model.py shows on the CPU that the guard scene contains what these tests rely on."""
import numpy as np
import pytest

import correct_model as C
import refresh_model as R

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE = -1, -2
FIELDS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")


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
    """The scene's points resident in one context, and the model's copy of the store."""

    def __init__(self, ctx, sc, max_points=512):
        from orbhip import localmap
        self.ex, self.m = ctx
        self.sc = sc
        self.lm = localmap.LocalMap(self.ex, max_points)          # (a new store: the last rig's is dropped)
        self.store = {k: np.array(sc[k]).copy() for k in FIELDS}
        self.lm.put(sc["keys"], *[self.store[k] for k in FIELDS])

    def get(self, which=None):
        return self.lm.map_get(self.sc["keys"] if which is None else self.sc["keys"][which])

    def check_store(self):
        g = self.get()
        for k in FIELDS:
            assert same(g[k], self.store[k]), k

    def sim3(self, P=None, nlevels=None, kfs=None):
        """The first P points of the scene through the call, compared with the model on the store as it stands; returns the outputs."""
        sc = self.sc
        P = len(sc["keys"]) if P is None else P
        sub = dict(sc, keys=sc["keys"][:P], corr=sc["corr"][:P], off=sc["off"][:P + 1], ref_pos=sc["ref_pos"][:P],
                   ref_level=sc["ref_level"][:P], nlevels=nlevels or sc["nlevels"], kfs=sc["kfs"] if kfs is None else kfs)
        want = C.correct_sim3(sub, {k: v[:P] for k, v in self.store.items()})
        got = self.lm.map_correct_sim3(sc["sf"], sub["nlevels"], sc["xf"], sub["kfs"], sub["keys"], sub["corr"], sub["off"],
                                       sc["obs_kf"][:sub["off"][P]], sub["ref_pos"], sub["ref_level"])
        for name, g, w in zip(("status", "pos", "normal", "min_dist", "max_dist"), got, want):
            assert same(g, w), (name, np.nonzero([not same(a, b) for a, b in zip(g, w)])[0][:8])
        for k, w in zip(("pos", "normal", "min_dist", "max_dist"), want[1:]):
            self.store[k][:P] = w
        self.check_store()                                         # write equals read-back, and nothing else moved
        return want

    def se3(self, P=None):
        sc = self.sc
        P = len(sc["keys"]) if P is None else P
        sub = dict(sc, keys=sc["keys"][:P], corr=sc["corr"][:P], pos_set=sc["pos_set"][:P])
        want = C.correct_se3(sub, {k: v[:P] for k, v in self.store.items()})
        got = self.lm.map_correct_se3(sc["xf"], sub["keys"], sub["corr"], sub["pos_set"])
        assert same(got[0], want[0]) and same(got[1], want[1]), np.nonzero([not same(a, b) for a, b in zip(got[1], want[1])])[0][:8]
        self.store["pos"][:P] = want[1]
        self.check_store()
        return want


# ---- orbhip_map_correct_sim3 ----
@pytest.mark.parametrize("P", [1, 15, 16, 17, 300])
def test_batch_sizes_at_the_block_edge(ctx, P):
    rig = Rig(ctx, C.make_scene(41, nkf=20, K=5, P=300))
    status = rig.sim3(P)[0]
    assert set(status.tolist()) <= {1, 3} and (P < 15 or (status == 3).sum() >= P // 2)
    rig.sim3(P)                                                     # on the corrected store: moved once more, from where it stands


def test_list_lengths_at_the_round_edges(ctx):
    lengths = [0, 1, 2, 15, 16, 17, 33]
    sc = C.make_scene(42, nkf=40, K=5, P=35, lengths=lengths)
    assert sorted(set(np.diff(sc["off"]).tolist())) == lengths
    status = Rig(ctx, sc).sim3()[0]
    assert (status == np.where(np.diff(sc["off"]) > 0, 3, 1)).all()


@pytest.mark.parametrize("K", [1, 2, 5])
def test_corrected_key_frames(ctx, K):
    sc = C.make_scene(43 + K, nkf=9, K=K, P=70)
    assert sorted(sc["kfs"]["rank"][sc["kfs"]["rank"] >= 0].tolist()) == list(range(K))
    Rig(ctx, sc).sim3()


def ranks_scene():
    """Key frames 1..5 corrected in that order, 0, 6 and 7 not.  For corr = 1, 2, 3 a point seen from ranks -1, corr - 1, corr,
    corr + 1 and -1, with the reference observer first, last and at rank corr - 1."""
    sc = C.make_scene(44, nkf=8, K=5, P=9, lengths=[5])
    sc["kfs"]["rank"] = [-1, 0, 1, 2, 3, 4, -1, -1]
    p = 0
    for c in (1, 2, 3):
        for ref in (0, 4, 1):
            a = sc["off"][p]
            sc["obs_kf"][a:a + 5] = [0, c, c + 1, c + 2, 6]        # ranks -1, c - 1, c, c + 1, -1: ascending key frame
            sc["corr"][p], sc["ref_pos"][p] = c, ref
            p += 1
    return sc


def test_observers_around_the_points_own_rank(ctx):
    sc = ranks_scene()
    want = Rig(ctx, sc).sim3()
    for variant in ("all_after", "all_before", "own_after"):       # what the device agreed with is none of these, at any point
        other = C.correct_sim3(sc, variant=variant)
        assert all(not same(want[2][p], other[2][p]) for p in range(9)), variant
    after = C.correct_sim3(sc, variant="all_after")
    before = C.correct_sim3(sc, variant="all_before")
    at_ref = [p for p in range(9) if sc["ref_pos"][p] == 1]         # the reference observer stands at rank corr - 1: moved already
    assert all(want[4][p] == after[4][p] and want[4][p] != before[4][p] for p in at_ref)


@pytest.mark.parametrize("nlevels", [1, 8, 16])
def test_ref_level_at_both_ends(ctx, nlevels):
    for level in sorted({0, nlevels - 1}):
        sc = C.make_scene(45 + level, nkf=6, K=2, P=20, lengths=[3, 1, 4], nlevels=nlevels, level=level)
        rig = Rig(ctx, sc)
        rig.sim3()
        assert same(rig.store["min_dist"], (rig.store["max_dist"] / sc["sf"][nlevels - 1]).astype(f32))


def test_bad_point_and_empty_list_in_the_middle(ctx):
    sc = C.make_scene(46, nkf=8, K=3, P=40, lengths=[4, 2, 0, 5, 1], bad_points=(6, 18))
    rig = Rig(ctx, sc)
    before = rig.get([6, 18])
    status = rig.sim3()[0]
    want = np.where(np.arange(40) % 5 == 2, 1, 3)
    want[[6, 18]] = 0
    assert (status == want).all()
    after = rig.get([6, 18])
    assert all(same(before[k], after[k]) for k in before)
    empty = np.arange(40) % 5 == 2
    g = rig.get()
    assert same(g["normal"][empty], sc["normal"][empty]) and same(g["max_dist"][empty], sc["max_dist"][empty])
    assert not same(g["pos"][empty], sc["pos"][empty])              # SetWorldPos, then UpdateNormalAndDepth returns early


def test_null_outputs(ctx):
    sc = C.make_scene(47, nkf=8, K=3, P=33)
    rig = Rig(ctx, sc)
    want = C.correct_sim3(sc)
    got = rig.lm.map_correct_sim3(sc["sf"], sc["nlevels"], sc["xf"], sc["kfs"], sc["keys"], sc["corr"], sc["off"], sc["obs_kf"],
                                  sc["ref_pos"], sc["ref_level"], want=False)
    assert same(got[0], want[0]) and all(g is None for g in got[1:])
    g = rig.get()
    assert same(g["pos"], want[1]) and same(g["normal"], want[2]) and same(g["min_dist"], want[3]) and same(g["max_dist"], want[4])


def test_guard_scene(ctx):
    sc, se3 = C.guard_scene(), C.guard_se3_scene()
    cnt = C.guard_counts(sc, se3)
    assert all(v >= 1 for v in cnt.values()), cnt
    Rig(ctx, sc).sim3()
    Rig(ctx, se3).se3()


def test_flags_generation_descriptors_and_rows_untouched(ctx):
    sc = C.make_scene(48, nkf=8, K=3, P=50)
    rig = Rig(ctx, sc)
    again = sc["keys"][10:20]
    rig.lm.erase(again)                                             # their slots' generations move on
    rig.lm.put(again, *[rig.store[k][10:20] for k in FIELDS])
    rig.lm.kf_init(4, 64)
    rig.lm.kf_put(0x900, sc["keys"][:30])
    rig.lm.kf_put(0x901, sc["keys"][25:])
    before = rig.lm.collect([0x900, 0x901], 64)
    assert len(before) == 50
    rig.sim3()
    assert same(rig.lm.collect([0x900, 0x901], 64), before)
    g = rig.get()
    assert same(g["flags"], sc["flags"]) and same(g["desc"], sc["desc"])
    se3 = C.make_se3_scene(48, K=3, P=50)
    rig2 = Rig(ctx, se3)
    rig2.lm.kf_init(4, 64)
    rig2.lm.kf_put(0x900, se3["keys"])
    before = rig2.lm.collect([0x900], 64)
    rig2.se3()
    assert same(rig2.lm.collect([0x900], 64), before) and same(rig2.get()["desc"], se3["desc"])


def test_search_after_correct_equals_search_after_put(ctx):
    """orbhip_search_local_points over the corrected store and over a second store that orbhip_map_put filled with the model's values."""
    from orbhip import localmap
    sc = C.make_scene(49, nkf=12, K=4, P=200, lengths=[3, 5, 2, 7])
    for k in ("Ow_before", "Ow_after"):
        sc["kfs"][k] *= f32(0.2)                                    # observers near the frame's camera: the points are seen from the front
    rig = Rig(ctx, sc)
    rig.sim3()
    rng = np.random.RandomState(5)
    n, FRAME = 400, 0x7000
    kps = np.zeros(n, R.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"], kps["size"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.randint(0, 8, n), 31
    fdesc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    fdesc[:200] = sc["desc"]
    pos = rig.store["pos"]
    kps["x"][:200] = np.clip(300 * pos[:, 0] / pos[:, 2] + 320, 1, 638)
    kps["y"][:200] = np.clip(300 * pos[:, 1] / pos[:, 2] + 240, 1, 478)
    rig.m.drop_set(0)
    rig.m.put_set(FRAME, kps, fdesc, None, (0.0, 0.0, 64 / 640.0, 48 / 480.0))
    cam = localmap.camera(np.eye(3), np.zeros(3), np.zeros(3), 300, 300, 320, 240, 0, (0, 640, 0, 480), sc["sf"][:8], np.log(f32(1.2)), 0.5, 3.0)
    skip = np.zeros(200, np.uint8)
    a = rig.lm.search(FRAME, n, cam, sc["keys"], skip)
    assert a[1] >= 20                                               # points in view: the corrected positions, normals and ranges are read
    second = localmap.LocalMap(rig.ex, 512)
    second.put(sc["keys"], *[rig.store[k] for k in FIELDS])
    b = second.search(FRAME, n, cam, sc["keys"], skip)
    assert same(a[0], b[0]) and a[1:3] == b[1:3] and same(a[3], b[3])


def test_refresh_after_the_call_equals_a_call_at_the_final_centres(ctx):
    """Once every SetPose has happened, orbhip_map_refresh with ORBHIP_REFRESH_NORMAL at the final camera centres gives what the call
    itself gives when nobody is corrected (every rank -1) and Ow_before already holds those centres."""
    from orbhip import localmap
    nlevels = 8
    sc = C.make_scene(50, nkf=10, K=4, P=80, nlevels=nlevels)
    final = np.where((sc["kfs"]["rank"] >= 0)[:, None], sc["kfs"]["Ow_after"], sc["kfs"]["Ow_before"])
    ex, m = ctx
    m.drop_set(0)
    assert m.set_limit(96) == 96
    kps = np.zeros(16, R.KP_DTYPE)                                  # feature i of every set sits on octave i % nlevels
    kps["x"], kps["y"], kps["size"], kps["octave"] = np.arange(16) * 7 + 5, 9, 31, np.arange(16) % nlevels
    rkfs = np.zeros(10, localmap.REFRESH_KF_DTYPE)
    rkfs["set_key"], rkfs["Ow"] = np.arange(10) + 0x5100, final
    for k in rkfs["set_key"]:
        m.put_set(int(k), kps, np.zeros((16, 32), np.uint8))
    obs_idx = np.zeros(len(sc["obs_kf"]), np.int32)
    live = np.diff(sc["off"]) > 0
    obs_idx[(sc["off"][:-1] + sc["ref_pos"])[live]] = sc["ref_level"][live]   # the reference observer's feature has the octave ref_level
    rig = Rig(ctx, sc)
    seq = rig.sim3()
    got = rig.lm.map_refresh(sc["sf"], nlevels, localmap.REFRESH_NORMAL, rkfs, sc["keys"], sc["off"], sc["obs_kf"], obs_idx, sc["ref_pos"])
    still = sc["kfs"].copy()
    still["rank"], still["Ow_before"] = -1, final
    rig2 = Rig(ctx, sc)
    want = rig2.sim3(kfs=still)
    assert same(want[1], seq[1]) and not same(want[2], seq[2])      # the same positions; the sequence saw other centres
    assert same(got[3], want[2]) and same(got[4], want[3]) and same(got[5], want[4])
    assert all(same(a, b) for a, b in zip(rig.get().values(), rig2.get().values()))


# ---- orbhip_map_correct_se3 ----
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_se3_batch_sizes_at_the_block_edge(ctx, P):
    rig = Rig(ctx, C.make_se3_scene(51, K=7, P=257, bad_points=(0, 100)))
    status = rig.se3(P)[0]
    assert status[0] == 0 and (status[1:] == 1).sum() >= P - 2


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("mode", ["set", "move", "mixed"])
def test_se3_modes(ctx, mode, K):
    sc = C.make_se3_scene(52 + K, K=K, P=90, mode=mode)
    n_set = int((sc["corr"] == -1).sum())
    assert n_set == 90 if mode == "set" else n_set == 0 if mode == "move" else 0 < n_set < 90
    rig = Rig(ctx, sc)
    rig.se3()
    g = rig.get()
    assert same(g["normal"], sc["normal"]) and same(g["min_dist"], sc["min_dist"]) and same(g["max_dist"], sc["max_dist"])   # position only
    if mode == "move":                                              # pos_set may be NULL when nothing reads it
        got = Rig(ctx, sc).lm.map_correct_se3(sc["xf"], sc["keys"], sc["corr"], None)
        assert same(got[1], rig.store["pos"])
    st, pos = Rig(ctx, sc).lm.map_correct_se3(sc["xf"], sc["keys"], sc["corr"], sc["pos_set"], want=False)
    assert pos is None and (st == 1).all()


# ---- errors: provoked by arguments alone, outputs and store unchanged ----
def test_sim3_errors_change_nothing(ctx):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    sc = C.make_scene(53, nkf=6, K=3, P=12, lengths=[3, 2, 4], nlevels=8)
    sc["ref_level"][5] = 7
    rig = Rig(ctx, sc)
    L, h = capi.load(), rig.ex.handle
    n = 12

    def call(nlevels=8, K=3, kfs=None, P=n, **kw):
        prm = np.zeros(1, localmap.REFRESH_PARAMS_DTYPE)
        prm["scale_factors"][0], prm["nlevels"] = sc["sf"], nlevels
        kfs = np.ascontiguousarray(sc["kfs"] if kfs is None else kfs, localmap.CORRECT_KF_DTYPE)
        xf = np.ascontiguousarray(sc["xf"], localmap.CORRECT_XF_DTYPE)
        a = [np.ascontiguousarray(kw.get(k, sc[k]), t) for k, t in (("keys", np.uint64), ("corr", np.int32), ("off", np.int32),
                                                                    ("obs_kf", np.int32), ("ref_pos", np.int32), ("ref_level", np.uint8))]
        m = max(P, 1)
        status = np.full(m, 0x5A, np.uint8)
        outs = [np.full((m, 3), 7, f32), np.full((m, 3), 7, f32), np.full(m, 7, f32), np.full(m, 7, f32)]
        rc = L.orbhip_map_correct_sim3(h, _p(prm), K, _p(xf), len(kfs), _p(kfs), P, *[_p(x) for x in a], _p(status), *[_p(x) for x in outs])
        if rc != 0:                                                 # a failed call changes nothing: neither the outputs nor the store
            assert (status == 0x5A).all() and all((o == 7).all() for o in outs)
            rig.check_store()
        return rc

    def edit(name, at, value):
        a = sc[name].copy()
        a[at] = value
        return a

    def with_rank(i, r):
        k = sc["kfs"].copy()
        k["rank"][i] = r
        return k

    corrected = np.nonzero(sc["kfs"]["rank"] >= 0)[0]
    assert call(keys=edit("keys", 4, 0x999999)) == E_ARG and call(keys=edit("keys", 4, 0)) == E_ARG      # an unknown point key
    assert call(keys=edit("keys", 4, sc["keys"][9])) == E_ARG                                             # a key twice
    assert call(corr=edit("corr", 2, 3)) == E_ARG and call(corr=edit("corr", 2, -1)) == E_ARG
    assert call(obs_kf=edit("obs_kf", 5, 6)) == E_ARG and call(obs_kf=edit("obs_kf", 5, -1)) == E_ARG
    assert call(ref_pos=edit("ref_pos", 0, 3)) == E_ARG and call(ref_pos=edit("ref_pos", 1, -1)) == E_ARG  # (list 0 has 3 rows)
    assert call(nlevels=7) == E_ARG                                 # point 5 names level 7
    assert call(nlevels=0) == E_ARG and call(nlevels=17) == E_ARG
    assert call(off=edit("off", 0, 1)) == E_ARG and call(off=edit("off", 3, sc["off"][2] - 1)) == E_ARG
    assert call(kfs=with_rank(0, 3)) == E_ARG and call(kfs=with_rank(0, -2)) == E_ARG
    assert call(kfs=with_rank(corrected[0], sc["kfs"]["rank"][corrected[1]])) == E_ARG                     # one rank twice
    assert call(K=0) == E_ARG
    big = np.zeros(1 << 20, np.int32)
    assert call(P=1, off=[0, 1 << 20], obs_kf=big, ref_pos=[0], keys=sc["keys"][:1], corr=[0], ref_level=[0]) == E_SIZE
    assert call(P=0) == 0 and call(P=0, K=0) == 0
    empty = np.zeros(13, np.int32)                                  # ref_pos is not read for an empty list
    rig.check_store()
    rig.sim3()                                                      # and the call still gives the model's answer
    sc2 = dict(sc, off=empty, obs_kf=np.zeros(0, np.int32), ref_pos=np.full(12, 99, np.int32))
    Rig(ctx, sc2).sim3()


def test_se3_errors_change_nothing(ctx):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    sc = C.make_se3_scene(54, K=3, P=12, mode="mixed")
    assert (sc["corr"] == -1).any() and (sc["corr"] >= 0).any()
    rig = Rig(ctx, sc)
    L, h = capi.load(), rig.ex.handle

    def call(K=3, P=12, pos_set=True, **kw):
        xf = np.ascontiguousarray(sc["xf"], localmap.CORRECT_SE3_DTYPE)
        keys, corr = np.ascontiguousarray(kw.get("keys", sc["keys"]), np.uint64), np.ascontiguousarray(kw.get("corr", sc["corr"]), np.int32)
        status, pos = np.full(12, 0x5A, np.uint8), np.full((12, 3), 7, f32)
        rc = L.orbhip_map_correct_se3(h, K, _p(xf), P, _p(keys), _p(corr), _p(sc["pos_set"]) if pos_set else None, _p(status), _p(pos))
        if rc != 0:
            assert (status == 0x5A).all() and (pos == 7).all()
            rig.check_store()
        return rc

    def edit(name, at, value):
        a = sc[name].copy()
        a[at] = value
        return a

    assert call(keys=edit("keys", 4, 0x999999)) == E_ARG and call(keys=edit("keys", 4, sc["keys"][9])) == E_ARG
    assert call(corr=edit("corr", 2, 3)) == E_ARG and call(corr=edit("corr", 2, -2)) == E_ARG
    assert call(K=2, corr=edit("corr", 2, 2)) == E_ARG and call(K=-1) == E_ARG
    assert call(pos_set=False) == E_ARG                             # a corr of -1 and nowhere to take the position from
    assert call(P=0) == 0
    rig.check_store()
    rig.se3()
