"""orbhip_map_kf_levels / orbhip_map_cull on the device against the model of KeyFrameCulling's loop on observation maps
(tests/cull_model.py): exact counts, verdicts and entry states, for both values of `monocular`, on the smallest tables that tell
the two sides of each comparison apart (csrc/k_cull.hip: 64 entries per trip of a row, four rows per block).  After every call,
failing ones included, the mark words must be zero again: an orbhip_map_vote gives its model's answer and a second orbhip_map_cull
repeats the first."""
import numpy as np
import pytest

import cull_model as UM
import localmap_collect_model as CM

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG = r"\(-1\)"
MAX_KFS, MAX_ROW = 12, 130
LB = UM.level_byte


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    yield e
    e.close()


class Rig:
    """A store of points without geometry (the counts read flags alone), a key-frame table with levels, and the model's world."""

    def __init__(self, ex, max_points=512, max_kfs=MAX_KFS, max_row=MAX_ROW):
        from orbhip import localmap
        self.lm = localmap.LocalMap(ex, max_points, max_kfs, max_row)
        self.w, self.lv = CM.World(), UM.Levels()

    def add_points(self, keys, bad=None):
        keys = np.asarray(keys, np.uint64)
        n = len(keys)
        bad = np.zeros(n, bool) if bad is None else np.asarray(bad, bool)
        self.lm.put(keys, np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.ones(n, f32), np.ones(n, f32), np.zeros((n, 32), np.uint8),
                    np.where(bad, 3, 1).astype(np.uint8))
        for k, b in zip(keys, bad):
            self.w.add_point(int(k), b)

    def put_kf(self, kf, row, levels=None, send_levels=True):
        levels = [LB(0)] * len(row) if levels is None else [int(b) for b in levels]
        assert len(levels) == len(row)
        self.lm.kf_put(kf, np.asarray(row, np.uint64))
        self.w.put_kf(kf, row)
        self.lv.put(kf, levels)
        if send_levels:
            self.lm.kf_levels([kf], [levels])

    def frame(self):
        return sorted(self.w.points)


def _raises(code, f, *a, **kw):
    from orbhip import capi
    with pytest.raises(capi.OrbHipError, match=code) as e:
        f(*a, **kw)
    return e.value


def _marks_clean(rig):
    frame = rig.frame()
    gk, gc = rig.lm.vote(np.asarray(frame, np.uint64))
    assert [(int(k), int(c)) for k, c in zip(gk, gc)] == CM.vote(rig.w, frame)


def check(rig, cands, th_obs=3):
    """Both values of monocular against the model, the marks afterwards and the repeat.  Returns {monocular: (counts, redundant)}."""
    cands = [int(k) for k in cands]
    out = {}
    for mono in (True, False):
        wc, wr, ws = UM.cull(rig.w, rig.lv, cands, mono, th_obs)
        counts, red, st = rig.lm.cull(cands, mono, th_obs, want_entries=True)
        for k, kf in enumerate(cands):
            got = [int(x) for x in st[k]]
            want = ws[k] + [0] * (st.shape[1] - len(ws[k]))
            assert got == want, "key frame %d, monocular %d: entries %s differ" % (kf, mono, [i for i in range(len(got)) if got[i] != want[i]])
        assert [tuple(int(x) for x in c) for c in counts] == wc
        assert [bool(r) for r in red] == wr
        _marks_clean(rig)
        c2, r2 = rig.lm.cull(cands, mono, th_obs)                  # without entry states: the same counts, and the repeat
        assert (c2 == counts).all() and (r2 == red).all()
        out[mono] = (wc, wr)
    return out


def _failed_call_left_alone(e):
    counts, red, st = e.outputs
    assert (counts == -7).all() and (red == 77).all() and (st is None or (st == 77).all())


def test_others_of_two_and_three_observations_of_three_and_four(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 8))
    st = LB(0, stereo=True)
    #               p1: 3 obs, 2 others | p2: 4 obs, 3 others | p3: two stereo observers: obs 4, others 1 | p4: as p2
    #               p5: stereo + 2: obs 4, others 2 | p6: stereo + 3: obs 5, others 3 | p7: the candidate alone
    rig.put_kf(2, [1, 2, 3, 4, 5, 6, 7], [LB(0), LB(0), st, LB(0), st, st, LB(0)])
    rig.put_kf(3, [1, 2, 3, 4, 5, 6], [LB(0), LB(0), st, LB(0), LB(0), LB(0)])
    rig.put_kf(4, [1, 2, 4, 5, 6])
    rig.put_kf(5, [2, 4, 6])
    got = check(rig, [2])
    assert got[True] == ([(7, 3)], [False]) and UM.cull(rig.w, rig.lv, [2], True)[2][0] == [1, 2, 1, 2, 1, 2, 1]
    assert check(rig, [2], th_obs=2)[True][0] == [(7, 5)]          # obs > 2 and others >= 2: p1, p2, p4, p5, p6
    assert check(rig, [2], th_obs=1)[True][0] == [(7, 6)]


def test_octaves_at_l_l_plus_one_l_plus_two_and_the_clamp_at_fifteen(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 7))
    # the candidate holds p1..p6 at octaves 3, 3, 0, 15, 14, 13; three observers each
    rig.put_kf(2, [1, 2, 3, 4, 5, 6], [LB(3), LB(3), LB(0), LB(15), LB(14), LB(13)])
    rig.put_kf(3, [1, 2, 3, 4, 5, 6], [LB(3), LB(4), LB(0), LB(15), LB(15), LB(15)])
    rig.put_kf(4, [1, 2, 3, 4, 5, 6], [LB(4), LB(4), LB(1), LB(15), LB(15), LB(14)])
    rig.put_kf(5, [1, 2, 3, 4, 5, 6], [LB(4), LB(5), LB(2), LB(0), LB(1), LB(14)])
    got = check(rig, [2])
    # p1: 3, 4, 4 <= 4 | p2: 5 > 4 | p3: 2 > 1 | p4: l = 15, everything counts | p5: 15 <= 15 | p6: 15 > 14
    assert UM.cull(rig.w, rig.lv, [2], True)[2][0] == [2, 1, 1, 2, 2, 1] and got[True][0] == [(6, 3)]
    check(rig, [3, 4, 5])


def test_own_entry_is_not_an_other_and_two_candidates_share_points(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 4))
    for kf in (2, 3, 4, 5):
        rig.put_kf(kf, [1, 2] if kf < 5 else [1])
    # p1: four observers, every candidate has three others; p2: three observers: obs 3
    got = check(rig, [2, 3, 4, 5])
    assert got[True][0] == [(2, 1), (2, 1), (2, 1), (1, 1)]
    # with th_obs 2, p2 (obs 3 > 2, others 2) is redundant for 2, 3 and 4: each subtracted itself, once
    assert check(rig, [2, 3, 4], th_obs=2)[True][0] == [(2, 2)] * 3
    rig.put_kf(6, [3])                                            # a point nobody else holds: others = 0, not -1 wrapped
    assert check(rig, [6], th_obs=1)[True][0] == [(1, 0)]


def test_the_far_bit(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 3))
    far = LB(0, far=True)
    rig.put_kf(2, [1, 2], [far, LB(0)])
    rig.put_kf(3, [1, 2], [far, far])
    rig.put_kf(4, [1, 2])
    rig.put_kf(5, [1, 2], [LB(0), far])
    got = check(rig, [2, 3, 4, 5])
    assert got[True][0] == [(2, 2)] * 4                            # monocular: ignored on both sides
    assert got[False][0] == [(1, 1), (0, 0), (2, 2), (1, 1)]       # skipped on the candidate's side, an observer on the other
    assert got[False][1] == [True, False, True, True]              # every entry far: nMPs == 0 and not redundant


def test_empty_bad_erased_and_stale_entries_and_an_erased_key_frame(ex):
    rig = Rig(ex)
    pts = list(range(1, 13))
    rig.add_points(pts, bad=[k == 3 for k in pts])
    for kf in (2, 3, 4, 5, 6):
        rig.put_kf(kf, [0] + pts + [0])
    base = check(rig, [2, 3])
    assert base[True][0] == [(11, 11)] * 2
    rig.lm.update_flags(np.asarray([4, 5], np.uint64), np.full(2, 3, np.uint8))   # points turn bad
    for k in (4, 5):
        rig.w.set_bad(k)
    assert check(rig, [2, 3])[True][0] == [(9, 9)] * 2
    gone = np.asarray([6, 7], np.uint64)                           # erased: every row keeps a stale entry
    slots_before = rig.lm.slots(gone)
    rig.lm.erase(gone)
    for k in gone:
        rig.w.erase_point(int(k))
    assert check(rig, [2, 3])[True][0] == [(7, 7)] * 2
    fresh = np.asarray([100, 101], np.uint64)                      # their slots go to new points, held by rows 2 and 3 alone
    rig.add_points(fresh)
    assert sorted(rig.lm.slots(fresh)) == sorted(slots_before)
    for kf in (2, 3):
        rig.lm.kf_set(kf, [0, 13], fresh)
        rig.w.set_entry(kf, 0, 100), rig.w.set_entry(kf, 13, 101)
    assert check(rig, [2, 3, 4])[True][0] == [(9, 7), (9, 7), (7, 7)]   # the stale entries of 4, 5, 6 do not observe 100, 101
    rig.lm.kf_erase(6)                                             # an erased key frame is no observer: obs 4, others 3 remain
    rig.w.erase_kf(6)
    assert check(rig, [2, 3, 4])[True][0] == [(9, 7), (9, 7), (7, 7)]
    rig.lm.kf_erase(5)
    rig.w.erase_kf(5)
    assert check(rig, [2, 3, 4])[True][0] == [(9, 0), (9, 0), (7, 0)]   # obs 3
    e = _raises(E_ARG, rig.lm.cull, [2, 5], True, want_entries=True)    # the erased key frame is no candidate either
    _failed_call_left_alone(e)
    _marks_clean(rig)
    rig.put_kf(7, [3, 4, 5])                                       # every entry bad
    assert check(rig, [7])[True] == ([(0, 0)], [False])


@pytest.mark.parametrize("n, r, verdict", [(10, 9, False), (10, 10, True), (20, 18, False), (20, 19, True)])
def test_nine_tenths(ex, n, r, verdict):
    rig = Rig(ex)
    rig.add_points(range(1, n + 1))
    rig.put_kf(2, list(range(1, n + 1)))
    for kf in (3, 4, 5):
        rig.put_kf(kf, list(range(1, r + 1)))
    assert check(rig, [2])[True] == ([(n, r)], [verdict])


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_row_lengths_around_the_trip_and_five_candidates(ex, n):
    rng = np.random.default_rng(n)
    rig = Rig(ex)
    pts = np.arange(1, n + 1)
    rig.add_points(pts)
    kfs = [2, 3, 5, 8, 13]                                         # five: a block of four waves and a partial successor
    for kf in kfs:
        rig.put_kf(kf, rng.permutation(pts), rng.integers(0, 3, n))
    got = check(rig, kfs)
    assert [c[0] for c in got[True][0]] == [n] * 5
    twice = check(rig, [5, 2, 5, 13, 5, 2])                        # a candidate given twice: the same answer twice
    assert twice[True][0][0] == twice[True][0][2] == twice[True][0][4] and twice[True][0][1] == twice[True][0][5]
    rig.lm.kf_put(21, np.asarray(pts[:3], np.uint64))              # a shorter row beside them, last entry of the table's sweep
    rig.w.put_kf(21, [int(p) for p in pts[:3]])
    rig.lv.put(21, [LB(2)] * 3)
    rig.lm.kf_levels([21], [[LB(2)] * 3])
    check(rig, kfs + [21])


def test_one_point_held_by_every_row_and_nothing_to_count(ex):
    rig = Rig(ex)
    rig.add_points([9])
    kfs = list(range(2, 2 + MAX_KFS))
    for i, kf in enumerate(kfs):
        rig.put_kf(kf, [0] * i + [9], [LB(0)] * i + [LB(i % 4, stereo=i % 3 == 0)])
    check(rig, kfs)
    counts, red = rig.lm.cull([], True)                            # K == 0
    assert len(counts) == 0 and len(red) == 0
    _marks_clean(rig)


def test_errors_of_both_calls_leave_everything_alone(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 9))
    for kf in (2, 3, 4, 5):
        rig.put_kf(kf, [1, 2, 3, 4])
    want = check(rig, [2, 3])
    assert list(rig.lm.kf_levels_missing()) == []
    ok = [LB(0)] * 4
    for keys, rows, off in (([2, 77], [ok, ok], None),             # an unknown key
                            ([2, 3, 2], [ok, ok, ok], None),       # a key twice
                            ([2], [[LB(0)] * (MAX_ROW + 1)], None),   # a segment longer than max_row
                            ([2, 3], [ok, ok], [0, 6, 4]),         # off not ascending
                            ([2, 3], [ok, ok], [1, 4, 8]),         # off not from 0
                            ([2], [[LB(0), 0x10, LB(0), LB(0)]], None),   # bit 4
                            ([2], [[LB(0), LB(0), LB(0), 0xA0 | 3]], None)):   # bit 5
        _raises(E_ARG, rig.lm.kf_levels, keys, rows, off)
        assert list(rig.lm.kf_levels_missing()) == []
        assert check(rig, [2, 3]) == want
    rig.lm.kf_levels([], [])                                       # m == 0
    for args in (([2, 77], True), ([2], True, 0), ([2], True, -3), ([2, 3] * 32769, True)):   # an unknown key; th_obs < 1; K > 65536
        _failed_call_left_alone(_raises(E_ARG, rig.lm.cull, *args, want_entries=True))
        _marks_clean(rig)
    # a live row that is no candidate and has no levels
    rig.put_kf(6, [5, 6], send_levels=False)
    assert list(rig.lm.kf_levels_missing()) == [6]
    _failed_call_left_alone(_raises(E_ARG, rig.lm.cull, [2, 3], True, want_entries=True))
    _marks_clean(rig)
    rig.lm.kf_levels([6], [[LB(0)] * 2])
    assert list(rig.lm.kf_levels_missing()) == [] and check(rig, [2, 3]) == want
    # levels survive a put of the same key; a row grown past its levels counts as without
    rig.put_kf(6, [6, 5], send_levels=False)
    assert list(rig.lm.kf_levels_missing()) == []
    check(rig, [2, 6])
    rig.put_kf(6, [6, 5, 7], send_levels=False)
    assert list(rig.lm.kf_levels_missing()) == [6]
    _failed_call_left_alone(_raises(E_ARG, rig.lm.cull, [2], False))
    _marks_clean(rig)
    rig.lm.kf_levels([6, 2], [[LB(1)] * 3, ok])
    rig.lv.put(6, [LB(1)] * 3)
    check(rig, [2, 6])
    # levels go with the row: erased, and the row taken by another key
    rig.lm.kf_erase(6)
    rig.w.erase_kf(6)
    assert list(rig.lm.kf_levels_missing()) == []
    rig.put_kf(9, [7, 8, 1], send_levels=False)
    assert list(rig.lm.kf_levels_missing()) == [9]
    rig.lm.kf_clear()
    assert list(rig.lm.kf_levels_missing()) == []
    rig.lm.kf_put(2, np.asarray([1, 2], np.uint64))
    assert list(rig.lm.kf_levels_missing()) == [2]


@pytest.fixture(scope="module")
def random_rig(ex):
    """12 key frames over 300 points, rows of 100, random levels and flags; built once, never edited."""
    rng = np.random.default_rng(22)
    rig = Rig(ex)
    keys = (np.arange(300, dtype=np.uint64) + np.uint64(1)) * np.uint64(7)
    rig.add_points(keys, rng.random(300) < 0.05)
    rig.kf_keys = [int(k) for k in rng.permutation(np.arange(12) + 2) * 5]
    popular = keys[:120]                                           # most rows share these: observers enough to be redundant
    for kf in rig.kf_keys:
        row = np.concatenate([rng.choice(popular, 70, replace=False), rng.choice(keys[120:], 30, replace=False)])
        row = rng.permutation(row)
        row[rng.random(100) < 0.08] = 0
        lv = rng.integers(0, 8, 100) | np.where(rng.random(100) < 0.3, 0x40, 0) | np.where(rng.random(100) < 0.2, 0x80, 0)
        rig.put_kf(kf, row, lv)
    return rig


def test_random_map_all_candidates(random_rig):
    got = check(random_rig, random_rig.kf_keys)
    for mono in (True, False):
        counts = got[mono][0]
        assert all(0 < r < m for m, r in counts)                   # both kinds of entry in every row
    assert got[True][0] != got[False][0]
    for th in (1, 2, 5):
        check(random_rig, random_rig.kf_keys, th_obs=th)
