"""orbhip_map_covis on the device against the model of KeyFrame::UpdateConnections on observation maps (tests/covis_model.py):
exact keys, weights and orders on small tables built to hit each edge of the kernels (csrc/k_covis.hip: 64 entries per trip of a
row, four rows per block, 32 queries per pass).  After every call, failing ones included, the mark words must be zero again: an
orbhip_map_vote gives the model's answer and a second orbhip_map_covis repeats the first."""
import numpy as np
import pytest

import covis_model as GM
import localmap_collect_model as CM

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
    """A store of points without geometry (the counts read flags alone), a key-frame table, and the model's world beside them."""

    def __init__(self, ex, max_points, max_kfs, max_row):
        from orbhip import localmap
        self.lm = localmap.LocalMap(ex, max_points, max_kfs, max_row)
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
        self.lm.kf_put(kf, np.asarray(row, np.uint64))
        self.w.put_kf(kf, row)


def _raises(code, f, *a, **kw):
    from orbhip import capi
    with pytest.raises(capi.OrbHipError, match=code) as e:
        f(*a, **kw)
    return e.value


def _plain(res):
    return [([int(k) for k in a], [int(x) for x in b], [int(k) for k in c]) for a, b, c in res]


def _marks_clean(rig, frame):
    gk, gc = rig.lm.vote(np.asarray(frame, np.uint64))
    assert [(int(k), int(c)) for k, c in zip(gk, gc)] == CM.vote(rig.w, frame)


def check(rig, queries, th=15, frame=()):
    """The call against the model, the marks afterwards, the repeat, and the call with room for one link less."""
    queries = [int(q) for q in queries]
    want = GM.covis(rig.w, queries, th)
    got = _plain(rig.lm.covis(queries, th))
    assert got == want
    for q, (keys, weights, order) in zip(queries, got):
        assert q not in keys and keys == sorted(keys) and all(x > 0 for x in weights)
    _marks_clean(rig, frame)
    total = sum(len(k) for k, _, _ in want)
    assert _plain(rig.lm.covis(queries, th, cap=total)) == want
    if total:
        e = _raises(E_CAPACITY, rig.lm.covis, queries, th, cap=total - 1)
        assert e.total == total
        off, nbr, w, order, nord = e.outputs
        assert (off == -1).all() and (nbr == 0).all() and (w == -1).all() and (order == -1).all() and (nord == -1).all()
        _marks_clean(rig, frame)
        assert _plain(rig.lm.covis(queries, th)) == want
    return want


LENGTHS = [0, 1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def big(ex):
    """70 key frames over 420 points, rows of every length around the 64-entry trip; built once, never edited."""
    rng = np.random.default_rng(20)
    rig = Rig(ex, 512, 72, 129)
    keys = (np.arange(420, dtype=np.uint64) + np.uint64(1)) * np.uint64(37)
    bad = rng.random(420) < 0.04
    rig.add_points(keys, bad)
    kfs = [int(k) for k in rng.permutation(np.arange(70) + 1) * 11]
    lens = list(LENGTHS) + [int(n) for n in rng.integers(2, 130, 64)]
    for kf, n in zip(kfs, lens):
        row = rng.choice(keys, n, replace=False)
        if n > 1:
            row[rng.random(n) < 0.1] = 0
        rig.put_kf(kf, row)
    rig.frame = [int(k) for k in rng.choice(keys, 90)]
    rig.kf_keys = kfs
    return rig


@pytest.mark.parametrize("nq", [1, 31, 32, 33, 65])
def test_pass_boundaries_and_row_lengths(big, nq):
    # the rows of the six lengths first: each is a query at every nq >= 6, the row of length 129 at nq = 1
    order = big.kf_keys[5:6] + big.kf_keys[:5] + big.kf_keys[6:]
    want = check(big, order[:nq], 15, big.frame)
    if nq >= 32:
        assert max(len(o) for _, _, o in want) >= 3 and any(len(k) > len(o) > 0 for k, _, o in want)   # links on both sides of th
    if nq >= 6:
        assert want[1] == ([], [], [])                                # the empty row


def test_thresholds_and_a_batch_equals_single_calls(big):
    qs = big.kf_keys[:40]
    for th in (1, 14, 15, 16, 1000):
        batched = _plain(big.lm.covis(qs, th))
        assert batched == GM.covis(big.w, qs, th)
        if th in (1, 15):
            assert batched == [_plain(big.lm.covis([q], th))[0] for q in qs]
    one = _plain(big.lm.covis(qs[:8], 1000))
    assert all(len(o) == (1 if k else 0) for k, _, o in one)           # no link reaches th: the single maximum
    _marks_clean(big, big.frame)


def test_a_key_twice_self_and_nothing_to_say(big):
    a, b, empty = big.kf_keys[7], big.kf_keys[9], big.kf_keys[0]
    qs = [a, b, a, empty, a] + big.kf_keys[10:40] + [b, empty]      # the copies fall into two passes
    want = check(big, qs, 15, big.frame)
    assert want[0] == want[2] == want[4] and want[1] == want[-2] and want[3] == want[-1] == ([], [], [])
    assert _plain(big.lm.covis([], 15)) == []
    _raises(E_ARG, big.lm.covis, [a, 424242], 15)                      # a key the table does not know
    _raises(E_ARG, big.lm.covis, [a], 0)                               # th >= 1
    _marks_clean(big, big.frame)
    assert _plain(big.lm.covis(qs, 15)) == want


@pytest.mark.parametrize("nrows", [1, 4, 5])
def test_tables_of_one_four_and_five_rows(ex, nrows):
    rng = np.random.default_rng(nrows)
    rig = Rig(ex, 128, nrows, 65)
    keys = np.arange(1, 101, dtype=np.uint64)
    rig.add_points(keys)
    kfs = [100 - 7 * i for i in range(nrows)]
    for kf in kfs:
        rig.put_kf(kf, rng.choice(keys, 65, replace=False))
    want = check(rig, kfs, 15, [int(k) for k in keys[:30]])
    assert all(len(k) == nrows - 1 for k, _, _ in want)
    check(rig, kfs[::-1] + kfs, 40, [int(k) for k in keys[:30]])


def test_a_query_that_shares_nothing_and_equal_weights(ex):
    rig = Rig(ex, 256, 8, 40)
    keys = np.arange(1, 201, dtype=np.uint64)
    rig.add_points(keys)
    rig.put_kf(5, keys[0:20])                       # shares nothing
    rig.put_kf(9, np.concatenate([keys[20:35], keys[40:55], keys[60:67]]))
    rig.put_kf(3, keys[20:35])                      # 15 with 9
    rig.put_kf(12, keys[40:55])                     # 15 with 9: the tie comes out as 12, 3
    rig.put_kf(7, keys[60:67])                      # 7 with 9
    rig.put_kf(2, np.concatenate([keys[100:107], keys[110:117]]))
    rig.put_kf(30, keys[100:107])                   # 7 and 7 with 2: no link reaches th, the lower key wins
    rig.put_kf(40, keys[110:117])
    want = check(rig, [5, 9, 2, 7], 15, [1, 25, 45, 65, 105])
    assert want == [([], [], []), ([3, 7, 12], [15, 7, 15], [12, 3]), ([30, 40], [7, 7], [30]), ([9], [7], [9])]


def test_bad_points_and_stale_entries(ex):
    rng = np.random.default_rng(8)
    rig = Rig(ex, 128, 16, 70)
    keys = np.arange(1, 101, dtype=np.uint64) * np.uint64(3)
    rig.add_points(keys)
    kfs = [4, 8, 15, 16, 23, 42]
    for kf in kfs:
        rig.put_kf(kf, np.concatenate([rng.choice(keys, 55, replace=False), np.zeros(15, np.uint64)]))
    frame = [int(k) for k in keys[::3]]
    base = check(rig, kfs, 15, frame)
    # points turn bad
    turned = keys[5:25]
    rig.lm.update_flags(turned, np.full(20, 3, np.uint8))
    for k in turned:
        rig.w.set_bad(int(k))
    bad = check(rig, kfs, 15, frame)
    assert bad != base
    # points erased: the rows that named them keep stale entries
    gone = keys[30:45]
    slots_before = rig.lm.slots(gone)
    rig.lm.erase(gone)
    for k in gone:
        rig.w.erase_point(int(k))
    erased = check(rig, kfs, 15, frame)
    assert erased != bad
    # their slots go to new points, held by two rows alone: the stale entries of the other rows must not count them
    fresh = np.arange(1000, 1015, dtype=np.uint64)
    rig.add_points(fresh)
    assert sorted(rig.lm.slots(fresh)) == sorted(slots_before)
    for kf in (8, 23):
        idx = list(range(55, 70))
        rig.lm.kf_set(kf, idx, fresh)
        for i, k in zip(idx, fresh):
            rig.w.set_entry(kf, i, int(k))
    reused = check(rig, kfs, 15, frame)
    assert dict(zip(reused[1][0], reused[1][1]))[23] == dict(zip(erased[1][0], erased[1][1]))[23] + 15
    # an erased key frame is nobody's neighbour, and no query
    rig.lm.kf_erase(15)
    rig.w.erase_kf(15)
    rest = [k for k in kfs if k != 15]
    after = check(rig, rest, 15, frame)
    assert all(15 not in k for k, _, _ in after)
    _raises(E_ARG, rig.lm.covis, [4, 15], 15)
    _marks_clean(rig, frame)
    # the store is cleared: every entry is stale; points put again resolve only in rows put again
    rig.lm.clear()
    rig.w.clear_points()
    assert _plain(rig.lm.covis(rest, 1)) == [([], [], [])] * len(rest)
    rig.add_points(keys[:60])
    for kf in (4, 8, 42):
        rig.put_kf(kf, rng.choice(keys[:60], 40, replace=False))
    final = check(rig, rest, 15, frame)
    assert [len(k) for k, _, _ in final] == [2, 2, 0, 0, 2]
