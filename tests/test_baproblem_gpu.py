"""orbhip_map_ba_problem on the device against the model of LocalBundleAdjustment's set-up on observation maps
(tests/baproblem_model.py): exact equality of the points, the offsets, the edges and the fixed key frames, on the smallest tables
that reach each path of csrc/k_baproblem.hip (64 entries per trip of a row, four rows per block, segments of up to one wave in
registers and longer ones in memory).  Key frames enter the table in DESCENDING key order, so the table's row order is never the
key order.  After every call, failing ones included, the mark words must be zero again (an orbhip_map_vote gives its model's
answer) and a second call repeats the first byte for byte; every cap is tried exact and one too small."""
import numpy as np
import pytest

import baproblem_model as BM
import localmap_collect_model as CM

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_CAPACITY = r"\(-1\)", r"\(-3\)"
MAX_KFS, MAX_ROW, MAX_POINTS = 80, 130, 512


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    yield e
    e.close()


class Rig:
    """A store of points without geometry (the problem reads flags alone), a key-frame table, and the model's world."""

    def __init__(self, ex, max_points=MAX_POINTS, max_kfs=MAX_KFS, max_row=MAX_ROW):
        from orbhip import localmap
        self.lm = localmap.LocalMap(ex, max_points, max_kfs, max_row)
        self.w = CM.World()

    def add_points(self, keys, bad=None):
        keys = np.asarray(list(keys), np.uint64)
        n = len(keys)
        bad = np.zeros(n, bool) if bad is None else np.asarray(bad, bool)
        self.lm.put(keys, np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.ones(n, f32), np.ones(n, f32), np.zeros((n, 32), np.uint8),
                    np.where(bad, 3, 1).astype(np.uint8))
        for k, b in zip(keys, bad):
            self.w.add_point(int(k), b)

    def put_kf(self, kf, row):
        self.lm.kf_put(kf, np.asarray(row, np.uint64))
        self.w.put_kf(kf, row)

    def put_kfs(self, rows):
        """{key: row} in descending key order: the smallest key takes the last row of the table."""
        for kf in sorted(rows, reverse=True):
            self.put_kf(kf, rows[kf])

    def erase_kf(self, kf):
        self.lm.kf_erase(kf)
        self.w.erase_kf(kf)


def _raises(code, f, *a, **kw):
    from orbhip import capi
    with pytest.raises(capi.OrbHipError, match=code) as e:
        f(*a, **kw)
    return e.value


def _marks_clean(rig):
    frame = sorted(rig.w.points)
    gk, gc = rig.lm.vote(np.asarray(frame, np.uint64))
    assert [(int(k), int(c)) for k, c in zip(gk, gc)] == CM.vote(rig.w, frame)


def _untouched(e):
    pts, off, edges, fixed = e.outputs
    assert (pts == 7).all() and (fixed == 7).all() and (off == -7).all() and (edges == -7).all()


def _as_lists(got):
    pts, off, edges, fixed = got
    return [int(k) for k in pts], [int(o) for o in off], [(int(a), int(b)) for a, b in edges], [int(k) for k in fixed]


def check(rig, kf_keys):
    """The call with exact caps against the model, the marks afterwards, the repeat, and every cap one too small.  Returns the
    model's answer."""
    kf_keys = [int(k) for k in kf_keys]
    want = BM.ba_problem(rig.w, kf_keys)
    pts, off, edges, fixed = want
    caps = (len(pts), len(edges), len(fixed))
    got = rig.lm.ba_problem(kf_keys, *caps)
    gl = _as_lists(got)
    assert gl[0] == pts
    assert gl[3] == fixed
    assert gl[1] == off
    assert gl[2] == edges, "edges differ first at %d" % next(i for i in range(len(edges)) if i >= len(gl[2]) or gl[2][i] != edges[i])
    assert all(b > a for a, b in zip(off, off[1:])) and off[-1] == len(edges)          # every point has an edge
    _marks_clean(rig)
    again = rig.lm.ba_problem(kf_keys, *caps)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    for which in range(3):
        if caps[which] == 0:
            continue
        small = list(caps)
        small[which] -= 1
        e = _raises(E_CAPACITY, rig.lm.ba_problem, kf_keys, *small)
        assert e.counts == caps
        _untouched(e)
        _marks_clean(rig)
    roomy = rig.lm.ba_problem(kf_keys, caps[0] + 5, caps[1] + 70, caps[2] + 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, roomy))
    return want


@pytest.mark.parametrize("n", [3, 4, 5, 31, 32, 33])
def test_live_rows_around_the_block_with_erased_rows_between(ex, n):
    rng = np.random.default_rng(n)
    rig = Rig(ex)
    pts = np.arange(1, 201)
    rig.add_points(pts)
    total = n + (n + 1) // 2                                       # every third row of the table is erased again
    keys = [10 + 3 * k for k in range(total)]
    rig.put_kfs({kf: rng.choice(pts, 40, replace=False) for kf in keys})
    by_row = sorted(keys, reverse=True)
    for kf in by_row[1::3][:total - n]:
        rig.erase_kf(kf)
    live = sorted(rig.w.kfs)
    assert len(live) == n
    local = [int(k) for k in rng.permutation(live)[:max(2, n // 3)]]
    _, _, edges, fixed = check(rig, local)
    assert len(fixed) == n - len(local)                            # 40 of 200 points a row: everybody shares with the local ones
    assert fixed != sorted(fixed) or n <= 4
    check(rig, live)                                               # every key frame local: nothing is fixed
    check(rig, live[::-1])


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 70])
def test_a_point_seen_by_k_key_frames(ex, k):
    rng = np.random.default_rng(k)
    rig = Rig(ex)
    rig.add_points(range(1, 41))
    keys = [int(x) for x in rng.permutation(np.arange(72)) + 100]  # 72 rows; the first k of this list see point 1
    rows = {}
    for j, kf in enumerate(keys):
        row = [int(p) for p in rng.choice(np.arange(2, 41), 6, replace=False)]
        if j < k:
            row.insert(int(rng.integers(0, 7)), 1)
        rows[kf] = row
    rig.put_kfs(rows)
    local = [keys[0], keys[71]]                                    # one that sees point 1 and (for k < 72) one that does not
    pts, off, edges, fixed = check(rig, local)
    j = pts.index(1)
    assert off[j + 1] - off[j] == k
    if k == 1:
        assert edges[off[j]] == (0, rows[keys[0]].index(1))       # a point only a local row holds


@pytest.mark.parametrize("n", [63, 64, 65, MAX_ROW])
def test_row_lengths_around_the_trip(ex, n):
    rng = np.random.default_rng(n)
    rig = Rig(ex)
    pts = np.arange(1, 2 * n + 1)
    rig.add_points(pts)
    rows = {kf: rng.permutation(pts)[:n] for kf in (2, 3, 5, 8, 13)}
    rows[21] = pts[:3]
    rig.put_kfs(rows)
    want = check(rig, [5, 13])
    assert len(want[3]) == 4
    check(rig, [21, 2])
    check(rig, [8])


def test_empty_row_doubled_key_bad_erased_and_reused_points_and_a_stranger(ex):
    rig = Rig(ex)
    pts = list(range(1, 21))
    rig.add_points(pts + [50, 51], bad=[k == 3 for k in pts] + [False, False])
    rows = {90: [], 80: [0] + pts[:10] + [0], 70: pts[5:15], 60: pts[8:20], 40: pts[:6], 30: [50, 51], 20: [20, 19]}
    rig.put_kfs(rows)
    local = [70, 90, 80, 70]                                       # an empty local row, a local key twice
    pts_w, off, edges, fixed = check(rig, local)
    assert 3 not in pts_w and 30 not in fixed                      # the bad point; a key frame sharing nothing
    assert fixed == [40, 60] and pts_w[0] == 6                     # 6 is seen by 40, 70, 80; 60 comes with 9
    assert all(kf != 3 for kf, _ in edges)                         # the second copy of 70 names nothing
    # points turn bad, points are erased: every row keeps a stale entry
    rig.lm.update_flags(np.asarray([7, 8], np.uint64), np.full(2, 3, np.uint8))
    for k in (7, 8):
        rig.w.set_bad(k)
    gone = np.asarray([9, 10], np.uint64)
    slots_before = rig.lm.slots(gone)
    rig.lm.erase(gone)
    for k in gone:
        rig.w.erase_point(int(k))
    check(rig, local)
    # their slots go to new points, held by rows 80 and 30 alone: the stale entries of 70 and 60 do not observe them
    fresh = np.asarray([100, 101], np.uint64)
    rig.add_points(fresh)
    assert sorted(rig.lm.slots(fresh)) == sorted(slots_before)
    rig.lm.kf_set(80, [0, 11], fresh)
    rig.w.set_entry(80, 0, 100), rig.w.set_entry(80, 11, 101)
    rig.lm.kf_set(30, [0], fresh[:1])
    rig.w.set_entry(30, 0, 100)
    pts_w, off, edges, fixed = check(rig, local)
    j = pts_w.index(100)
    assert off[j + 1] - off[j] == 2 and 30 in fixed
    j = pts_w.index(101)
    assert off[j + 1] - off[j] == 1                                # a point only a local row holds
    # an erased key frame observes nothing and is not fixed; as a local key frame it is an unknown key
    rig.erase_kf(60)
    assert 60 not in check(rig, local)[3]
    _untouched(_raises(E_ARG, rig.lm.ba_problem, [70, 60], 64, 512, 8))
    _marks_clean(rig)
    check(rig, [20])                                               # shares with 60 (gone) alone: no fixed key frame
    check(rig, [90])                                               # local rows without entries: nothing launched
    assert check(rig, [30, 90]) == ([100, 51], [0, 2, 3], [(0, 0), (2, 0), (0, 1)], [80])


def test_a_fixed_key_frame_first_met_at_the_last_edge(ex):
    rig = Rig(ex)
    rig.add_points(range(1, 9))
    rig.put_kfs({5: [1, 2, 3, 4, 5, 6, 7, 8], 7: [1, 2, 3], 9: [0, 0, 4, 5], 11: [0, 8]})
    pts, off, edges, fixed = check(rig, [5])
    assert fixed == [7, 9, 11] and edges[-1] == (3, 1) and [kf for kf, _ in edges].count(3) == 1
    pts, off, edges, fixed = check(rig, [5, 9])
    assert fixed == [7, 11] and edges[-1] == (3, 1)


def test_argument_errors_and_no_key_frames(ex):
    from orbhip import capi, localmap
    from orbhip.extractor import ORBextractor
    rig = Rig(ex)
    rig.add_points(range(1, 9))
    rig.put_kfs({2: [1, 2, 3, 4], 3: [3, 4, 5], 4: [5, 6]})
    want = check(rig, [3])
    for kfs in ([3, 77], [0], [2, 3] * 32769):                     # an unknown key, key 0, nkf > 65536
        _untouched(_raises(E_ARG, rig.lm.ba_problem, kfs, 64, 64, 8))
        _marks_clean(rig)
    for caps in ((-1, 64, 8), (64, -1, 8), (64, 64, -1)):
        _untouched(_raises(E_ARG, rig.lm.ba_problem, [3], *caps))
    L, h = capi.load(), ex.handle                                  # null pointers
    kk, p, o, e, f, n = (np.asarray([3], np.uint64), np.zeros(8, np.uint64), np.zeros(9, np.int32), np.zeros((8, 2), np.int32),
                         np.zeros(8, np.uint64), [capi.C.c_int(-7) for _ in range(3)])
    B = capi.C.byref
    ok = [h, 1, capi._p(kk), capi._p(p), 8, B(n[0]), capi._p(o), capi._p(e), 8, B(n[1]), capi._p(f), 8, B(n[2])]
    for hole in (2, 3, 5, 6, 7, 9, 10, 12):
        args = list(ok)
        args[hole] = None
        assert L.orbhip_map_ba_problem(*args) == -1
    assert L.orbhip_map_ba_problem(*ok) == 0 and [x.value for x in n] == [len(want[0]), len(want[2]), len(want[3])]
    assert check(rig, [3]) == want
    got = _as_lists(rig.lm.ba_problem([], 0, 0, 0))                # nkf == 0
    assert got == ([], [0], [], [])
    _marks_clean(rig)
    ex2 = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    try:
        bare = localmap.LocalMap.__new__(localmap.LocalMap)        # no store
        bare._L, bare._ctx = L, ex2
        _untouched(_raises(E_ARG, bare.ba_problem, [3], 8, 8, 8))
        _untouched(_raises(E_ARG, bare.ba_problem, [], 8, 8, 8))
        only_store = localmap.LocalMap(ex2, 16)                    # a store without a table
        _untouched(_raises(E_ARG, only_store.ba_problem, [3], 8, 8, 8))
    finally:
        ex2.close()


def test_sixty_local_rows_give_the_points_of_collect(ex):
    rng = np.random.default_rng(60)
    rig = Rig(ex)
    keys = (np.arange(MAX_POINTS - 12, dtype=np.uint64) + np.uint64(1)) * np.uint64(7)
    rig.add_points(keys, rng.random(len(keys)) < 0.05)
    kfs = [int(k) for k in rng.permutation(np.arange(72)) * 5 + 5]
    rows = {}
    for kf in kfs:
        row = rng.choice(keys, MAX_ROW, replace=False)
        row[rng.random(MAX_ROW) < 0.08] = 0
        rows[kf] = row
    rig.put_kfs(rows)
    local = kfs[:60]
    pts, off, edges, fixed = check(rig, local)
    assert [int(k) for k in rig.lm.collect(local, len(pts))] == pts
    assert len(fixed) == 12 and max(b - a for a, b in zip(off, off[1:])) > 20
