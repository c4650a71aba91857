"""The key-frame -> map-point table, orbhip_map_vote, orbhip_map_collect and orbhip_track_local_points on the device against the
independent model of the reference's two loops (tests/localmap_collect_model.py): exact keys, counts and order; the compaction on
both sides of its block size; stale row entries; the fused call against orbhip_search_local_points fed with the model's list."""
import numpy as np
import pytest

import localmap_collect_model as CM
import localmap_model as M
import localmap_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
FRAME = 77
BLOCK = 256          # COLLECT_BLOCK of csrc/k_localcollect.hip
E_ARG, E_CAPACITY = r"\(-1\)", r"\(-3\)"


class Rig:
    """One small context, a store of points without geometry (the union and the vote read flags alone) and the model's world."""

    def __init__(self, max_points, max_kfs, max_row):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.lm = localmap.LocalMap(self.ex, max_points, max_kfs, max_row)
        self.w = CM.World()

    def add_points(self, keys, bad=None):
        keys = np.asarray(keys, np.uint64)
        n = len(keys)
        bad = np.zeros(n, bool) if bad is None else np.asarray(bad, bool)
        self.lm.put(keys, np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.ones(n, f32), np.ones(n, f32), np.zeros((n, 32), np.uint8),
                    np.where(bad, 3, 1).astype(np.uint8))
        for k, b in zip(keys, bad):
            self.w.add_point(int(k), b)

    def put_kf(self, kf, row):
        self.lm.kf_put(kf, row)
        self.w.put_kf(kf, row)

    def state(self):
        return self.lm.info(), self.lm.kf_info()

    def close(self):
        self.ex.close()


def _raises(code, f, *a):
    from orbhip import capi
    with pytest.raises(capi.OrbHipError, match=code) as e:
        f(*a)
    return e.value


def _too_small(f, args, want_keys, want_counts=None):
    """f(*args) with room for one entry less than the answer: the error, the whole count, and the first cap entries filled."""
    e = _raises(E_CAPACITY, f, *args)
    part = e.partial if want_counts is None else e.partial[0]
    assert e.total == len(want_keys) and [int(k) for k in part] == [int(k) for k in want_keys[:-1]]
    if want_counts is not None:
        assert [int(c) for c in e.partial[1]] == [int(c) for c in want_counts[:-1]]


def test_vote_equals_the_observation_maps():
    rng = np.random.default_rng(31)
    rig = Rig(512, 48, 70)
    keys = (np.arange(300, dtype=np.uint64) + np.uint64(1)) * np.uint64(101)
    bad = rng.random(300) < 0.05
    bad[7] = True
    rig.add_points(keys, bad)
    kfs = [int(k) for k in (np.arange(40) + 1) * 13][::-1]          # put in descending key order
    lens = rng.integers(0, 71, 40)
    lens[3], lens[17], lens[29] = 0, 70, 1
    for kf, n in zip(kfs, lens):
        row = rng.choice(keys, n, replace=False)
        row[rng.random(n) < 0.2] = 0
        rig.put_kf(kf, row)
    assert rig.lm.kf_info() == (40, 48, 70)
    erased = int(keys[11])
    frame = np.concatenate([rng.choice(keys, 120), np.zeros(9, np.uint64), keys[:25], keys[:25],
                            np.array([424243, keys[7], erased], np.uint64)])
    rng.shuffle(frame)
    rig.lm.erase([erased])
    rig.w.erase_point(erased)
    want = CM.vote(rig.w, frame)
    assert len(want) >= 30 and max(c for _, c in want) >= 8
    gk, gc = rig.lm.vote(frame)
    assert [(int(k), int(c)) for k, c in zip(gk, gc)] == want
    assert list(gk) == sorted(gk)
    before = rig.state()
    _too_small(rig.lm.vote, (frame, len(want) - 1), [k for k, _ in want], [c for _, c in want])
    assert rig.state() == before
    for _ in range(2):                                                # the marks are cleared: a second vote equals a fresh one
        gk2, gc2 = rig.lm.vote(frame, len(want))
        assert np.array_equal(gk2, gk) and np.array_equal(gc2, gc)
    # a bad and an erased point alone vote for nothing; an empty frame; only zeros
    for fr in ([keys[7], erased], [], [0, 0, 0]):
        gk3, gc3 = rig.lm.vote(np.array(fr, np.uint64))
        assert len(gk3) == 0 and CM.vote(rig.w, fr) == []
    rig.close()


def _union_rows(rng, keys, total):
    """Six rows of `total` entries in all: A1, an empty row, B1, a row of 41 zeros, A2, B2, where A1 + A2 and B1 + B2 each hold
    every point of `keys[:m]` once (two different orders), so that every point is shared by two rows."""
    m = (total - 41 - 10) // 2
    z = total - 41 - 2 * m
    pa, pb = rng.permutation(keys[:m]), rng.permutation(keys[:m])
    za = z // 2
    a = np.insert(pa, np.sort(rng.integers(0, m + 1, za)), 0)
    b = np.insert(pb, np.sort(rng.integers(0, m + 1, z - za)), 0)
    ca, cb = int(len(a) * 0.45), int(len(b) * 0.6)
    rows = [a[:ca], np.zeros(0, np.uint64), b[:cb], np.zeros(41, np.uint64), a[ca:], b[cb:]]
    assert sum(len(r) for r in rows) == total
    return rows


@pytest.mark.parametrize("total", [BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1])
def test_union_is_the_reference_list_element_for_element(total):
    from orbhip import capi
    rng = np.random.default_rng(100 + total)
    rig = Rig(512, 8, 3 * BLOCK)
    keys = (rng.permutation(400).astype(np.uint64) + np.uint64(1)) * np.uint64(17)
    bad = rng.random(400) < 0.06
    rig.add_points(keys, bad)
    rows = _union_rows(rng, keys, total)
    kfs = [5, 9, 2, 14, 3, 8]
    for kf, row in zip(kfs, rows):
        rig.put_kf(kf, row)
    want = CM.collect(rig.w, kfs)
    m = (total - 51) // 2
    assert len(want) == int((~bad[:m]).sum()) and len(want) > 60
    if total > BLOCK:      # first and second occurrence of a point in different scan blocks, the survivor in the lower and the higher
        flat = np.concatenate(rows)
        pos = {}
        for p, k in enumerate(flat):
            if k:
                pos.setdefault(int(k), []).append(p // BLOCK)
        assert any(b[0] != b[1] for b in pos.values())
    got = rig.lm.collect(kfs, total)
    assert [int(k) for k in got] == want
    assert [int(k) for k in rig.lm.collect(kfs, total)] == want                         # first[] restored
    rev = [int(k) for k in rig.lm.collect(kfs[::-1], total)]
    assert rev == CM.collect(rig.w, kfs[::-1]) and rev != want and sorted(rev) == sorted(want)
    assert [int(k) for k in rig.lm.collect(kfs + [kfs[0], kfs[4]], len(want))] == want   # a key frame twice; cap = exactly enough
    assert [int(k) for k in rig.lm.collect([kfs[1], kfs[3]], 4)] == []                   # the empty row and the row of zeros alone
    assert len(rig.lm.collect([], 4)) == 0                                              # nkf = 0
    before = rig.state()
    _raises(E_ARG, rig.lm.collect, kfs + [4242], total)
    _too_small(rig.lm.collect, (kfs, len(want) - 1), want)
    assert rig.state() == before
    assert [int(k) for k in rig.lm.collect(kfs, total)] == want
    gk, gc = rig.lm.vote(keys[:m])
    assert [(int(k), int(c)) for k, c in zip(gk, gc)] == CM.vote(rig.w, keys[:m])
    rig.close()


def _stale_sequence(rig, keys, kfs, clear):
    lm, w = rig.lm, rig.w
    cap = 64
    both = lambda: ([int(k) for k in lm.collect(kfs, cap)], [(int(k), int(c)) for k, c in zip(*lm.vote(keys))])
    assert both() == (CM.collect(w, kfs), CM.vote(w, keys))
    victim, fresh = int(keys[4]), 999983
    at = [(kf, w.kfs[kf].index(victim)) for kf in kfs if victim in w.kfs[kf]]
    assert len(at) >= 2
    slot = int(lm.slots([victim])[0])
    if clear:
        lm.clear()
        w.clear_points()
        assert both() == ([], [])
        rig.add_points(keys[::-1])           # the same keys again, other slots: no row names them until it is set again
        assert int(lm.slots([victim])[0]) != slot
        assert both() == ([], []) and CM.collect(w, kfs) == []
        kf, idx = at[0]
        lm.kf_set(kf, [idx], [victim])
        w.set_entry(kf, idx, victim)
        assert both() == ([victim], [(kf, 1)]) == (CM.collect(w, kfs), CM.vote(w, keys))
        return
    lm.erase([victim])
    w.erase_point(victim)
    got = both()
    assert got == (CM.collect(w, kfs), CM.vote(w, keys)) and victim not in got[0]
    rig.add_points([fresh])                  # takes the slot that was freed last
    assert int(lm.slots([fresh])[0]) == slot
    allkeys = np.concatenate([keys, np.array([fresh], np.uint64)])
    got = ([int(k) for k in lm.collect(kfs, cap)], [(int(k), int(c)) for k, c in zip(*lm.vote(allkeys))])
    assert got == (CM.collect(w, kfs), CM.vote(w, allkeys)) and victim not in got[0] and fresh not in got[0]
    kf, idx = at[1]
    lm.kf_set(kf, [idx], [fresh])
    w.set_entry(kf, idx, fresh)
    got = ([int(k) for k in lm.collect(kfs, cap)], [(int(k), int(c)) for k, c in zip(*lm.vote(allkeys))])
    want = CM.collect(w, kfs)
    assert got == (want, CM.vote(w, allkeys)) and fresh in want
    # at that index's position: between the survivors of its own row on either side of it
    mine = [k for k in w.kfs[kf] if k in want and all(k not in w.kfs[o] for o in kfs[:kfs.index(kf)])]
    assert fresh in mine and [k for k in want if k in mine] == mine


@pytest.mark.parametrize("clear", [False, True])
def test_stale_row_entries_never_resolve(clear):
    rng = np.random.default_rng(57)
    rig = Rig(64, 8, 24)
    keys = (np.arange(30, dtype=np.uint64) + np.uint64(1)) * np.uint64(19)
    rig.add_points(keys)
    kfs = [21, 22, 23]
    for kf in kfs:
        row = rng.permutation(keys)[:20]
        if keys[4] not in row:
            row[3] = keys[4]
        others = np.nonzero(row != keys[4])[0]
        row[others[rng.integers(0, len(others))]] = 0
        rig.put_kf(kf, row)
    _stale_sequence(rig, keys, kfs, clear)
    rig.close()


def test_error_paths_change_nothing():
    rng = np.random.default_rng(3)
    rig = Rig(64, 3, 10)
    keys = (np.arange(20, dtype=np.uint64) + np.uint64(1)) * np.uint64(23)
    rig.add_points(keys)
    rig.put_kf(1, keys[:10])
    rig.put_kf(2, np.concatenate([keys[5:12], np.zeros(2, np.uint64)]))
    lm = rig.lm
    snap = lambda: (rig.state(), list(lm.collect([1, 2], 32)), [list(x) for x in lm.vote(keys)])
    before = snap()
    _raises(E_ARG, lm.kf_put, 1, np.concatenate([keys[:3], np.array([555], np.uint64)]))     # a point the store does not know
    _raises(E_ARG, lm.kf_put, 3, keys[[0, 1, 0]])                                             # a point twice
    _raises(E_ARG, lm.kf_put, 3, keys[:11])                                                   # n > max_row
    _raises(E_ARG, lm.kf_put, 0, keys[:2])                                                    # key 0
    _raises(E_ARG, lm.kf_set, 2, [9], [keys[0]])                                              # outside the row (length 9)
    _raises(E_ARG, lm.kf_set, 2, [-1], [keys[0]])
    _raises(E_ARG, lm.kf_set, 2, [8], [keys[5]])                                              # already at index 0
    _raises(E_ARG, lm.kf_set, 2, [8], [777])
    _raises(E_ARG, lm.kf_set, 7, [0], [keys[0]])                                              # unknown key frame
    _raises(E_ARG, lm.collect, [1, 7], 32)
    _raises(E_CAPACITY, lm.collect, [1, 2], 11)
    lm.kf_erase(7)                                                                            # absent: no error
    assert snap() == before
    rig.put_kf(3, keys[12:14])
    _raises(E_CAPACITY, lm.kf_put, 4, keys[:2])                                               # the table is full
    assert rig.lm.kf_info() == (3, 3, 10)
    lm.kf_erase(3)
    assert snap() == before
    lm.kf_set(2, [8, 0], [keys[5], 0])       # moves a point inside the row in one call
    rig.w.set_entry(2, 0, 0)
    rig.w.set_entry(2, 8, int(keys[5]))
    assert [int(k) for k in lm.collect([2, 1], 32)] == CM.collect(rig.w, [2, 1])
    lm.kf_clear()
    assert lm.kf_info() == (0, 3, 10) and len(lm.vote(keys)[0]) == 0
    _raises(E_ARG, lm.collect, [1], 32)
    lm.kf_init(5, 12)                        # again: the old table is dropped
    assert lm.kf_info() == (0, 5, 12)
    rig.close()


def _cam_record(cam, th):
    from orbhip import localmap
    return localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                           cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], th)


@pytest.fixture(scope="module")
def fused_scene(oracle):
    """Points that compete for features (copies of the points in view with a few descriptor bits flipped) among the scene's
    others, dealt over 12 overlapping rows."""
    sc = scenes.make(oracle, "640x480", npoints=600)
    rng = np.random.default_rng(17)
    rec, code = M.frustum(sc["cam"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    src = np.nonzero(code == M.IN_VIEW)[0][:120]
    idx = np.concatenate([np.repeat(src, 3), np.arange(600)])
    pd = sc["pdesc"][idx].copy()
    for j in range(3 * len(src)):
        for b in rng.integers(0, 256, j % 3):
            pd[j, b >> 3] ^= np.uint8(1 << (b & 7))
    keys = (rng.permutation(len(idx)).astype(np.uint64) + np.uint64(1)) * np.uint64(13)
    flags = sc["flags"][idx].copy()
    flags[:3 * len(src)] = 1
    pts = dict(keys=keys, pos=sc["pos"][idx], normal=sc["normal"][idx], min_dist=sc["min_dist"][idx], max_dist=sc["max_dist"][idx],
               pdesc=pd, flags=flags)
    order = rng.permutation(len(idx))
    rows = [[] for _ in range(12)]
    for t, i in enumerate(order):
        for r in {t % 12, (t * 5 + 1) % 12, (t // 12) % 12}:
            rows[r].append(int(keys[i]))
            if rng.random() < 0.1:
                rows[r].append(0)
    return sc, pts, rows


@pytest.mark.parametrize("th,frame", [(1.0, True), (3.0, True), (5.0, True), (3.0, False)])
def test_fused_call_equals_collect_then_search(oracle, fused_scene, th, frame):
    from orbhip import localmap
    from orbhip.extractor import ORBextractor, ORBmatcher
    sc, pts, rows = fused_scene
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    m = ORBmatcher(0.8, False, ctx=ex)
    m.put_set(FRAME, sc["kps"], sc["desc"], None, sc["gp"])
    lm = localmap.LocalMap(ex, 2048, 16, max(len(r) for r in rows))
    lm.put(pts["keys"], pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["pdesc"], pts["flags"])
    w = CM.World()
    for k, fl in zip(pts["keys"], pts["flags"]):
        w.add_point(int(k), bool(fl & 2))
    kfs = [int(k) for k in (np.arange(12) + 1) * 7]
    for kf, row in zip(kfs, rows):
        lm.kf_put(kf, row)
        w.put_kf(kf, row)
    rng = np.random.default_rng(5)
    seen = np.concatenate([rng.choice(pts["keys"], 40, replace=False), np.array([31337, 0], np.uint64)])
    n = len(sc["kps"]) if frame else 0
    cam = _cam_record(sc["cam"], th)
    ur, occ = (sc["u_right"], sc["occupied"]) if frame else (None, None)
    winners = {}
    for name, order in (("fwd", kfs), ("rev", kfs[::-1])):
        want = CM.collect(w, order)
        skip = np.array(CM.skip_bytes(want, seen), np.uint8)
        assert 0 < skip.sum() <= 40 and len(want) > 700
        old = lm.search(FRAME if frame else 0, n, cam, np.array(want, np.uint64), skip, 0.8, ur, occ)
        for cap in (len(want), len(want) + 37):
            got = lm.track(FRAME if frame else 0, n, cam, order, seen, cap, 0.8, ur, occ)
            assert [int(k) for k in got[0]] == want
            assert got[1].tobytes() == old[0].tobytes()
            assert (got[2], got[3]) == (old[1], old[2]) and np.array_equal(got[4], old[3])
        assert old[1] > 100 and (not frame or old[2] > 0)         # (not a comparison of empty results)
        _too_small(lm.track, (FRAME if frame else 0, n, cam, order, seen, len(want) - 1, 0.8, ur, occ), want)
        assert [int(k) for k in lm.collect(order, len(want))] == want               # marks and first[] as they were
        winners[name] = np.where(old[3] >= 0, np.array(want, np.uint64)[np.maximum(old[3], 0)], 0) if frame else None
    if frame and th == 3.0:
        # the order matters in this scene: a feature goes to another point when the rows are reversed, here and in the model
        assert (winners["fwd"] != winners["rev"]).any()
        store = M.Store(2048)
        store.put(pts["keys"], pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], pts["pdesc"], pts["flags"])
        mw = {}
        for name, order in (("fwd", kfs), ("rev", kfs[::-1])):
            want = np.array(CM.collect(w, order), np.uint64)
            skip = np.array(CM.skip_bytes(want, seen), np.uint8)
            r = M.search_local_points(oracle, store, sc["cam"], th, want, skip, sc["kps"], sc["desc"], sc["gp"], 0.8, sc["u_right"],
                                      sc["occupied"])
            mw[name] = np.where(r[4] >= 0, want[np.maximum(r[4], 0)], 0)
            assert np.array_equal(mw[name], winners[name])
        assert (mw["fwd"] != mw["rev"]).any()
    _raises(E_ARG, lm.track, FRAME if frame else 0, n, cam, kfs + [99], seen, 4096, 0.8, ur, occ)
    got = lm.track(FRAME if frame else 0, n, cam, [], seen, 16, 0.8, ur, occ)
    assert len(got[0]) == 0 and got[2] == 0 and got[3] == 0 and (got[4] == -1).all()
    m.close()
    ex.close()
