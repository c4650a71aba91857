"""The device key-frame database (orbhip/kfdb.py over orbhip_kfdb_*) against tests/kfdb_model.py, the plain restatement of
src/KeyFrameDatabase.cc: candidate keys in order after every query, shared-word counts and float scores bit for bit."""
import numpy as np
import pytest

from kfdb_model import KF, Model

pytestmark = pytest.mark.gpu

RELOC, LOOP = 0, 1


@pytest.fixture(scope="module")
def env():
    from orbhip import distributed as D, synth
    from orbhip.extractor import ORBextractor
    from orbhip.vocabulary import ORBVocabulary
    ex = ORBextractor(1000, 1.2, 8, 20, 7, max_w=640, max_h=480, max_batch=1)
    voc = ORBVocabulary(ex)
    voc.loadFromBinaryBlob(D.make_synthetic_vocabulary(23, k=10, L=4))
    bows = []
    for seed in (3, 4, 5):
        for f in synth.make_frames(seed, 640, 480, 8):
            _, d = ex(f)
            (w, v), _ = voc.transform(d, 4)
            bows.append((w.astype(np.uint32), v))
    yield ex, voc, bows
    ex.close()


def _variant(rng, bow, keep=0.7):
    """a BowVector that shares part of `bow`'s words (L1-normalised, as transform makes them)"""
    w, v = bow
    m = rng.random(len(w)) < keep
    if not m.any():
        m[0] = True
    v2 = v[m] * (1.0 + 0.25 * rng.random(m.sum()))
    return w[m].copy(), v2 / np.abs(v2).sum()


def _db(env, max_kfs=4096, delta_max=0):
    from orbhip.kfdb import KeyFrameDatabase
    ex, voc, _ = env
    return KeyFrameDatabase(ex, voc.nwords, max_kfs=max_kfs, delta_max=delta_max)


def _keys(kfs):
    return [k.key for k in kfs]


def _check_score(db, model, mode, bow, excluded=()):
    keys, cnt, sc, minc = db.score(mode, bow, [k.key for k in excluded])
    want, wminc = model.score(mode, bow, excluded)
    assert list(keys) == [k for k, _, _ in want]
    assert list(cnt) == [c for _, c, _ in want]
    assert sc.tobytes() == np.array([s for _, _, s in want], np.float32).tobytes()
    assert minc == wminc or not want


def _set_covis(db, rng, kf, live):
    others = [k for k in live if k is not kf]
    n = min(len(others), int(rng.integers(0, 11)))
    idx = rng.choice(len(others), n, replace=False) if n else []
    kf.covis = [others[i] for i in idx]          # "weighted order": the order drawn stands for decreasing weight
    db.set_covis(kf.key, [k.key for k in kf.covis])


@pytest.mark.parametrize("delta_max", [1, 16, 0])
def test_interleaved_sequence_matches_the_reference(env, delta_max):
    _, voc, bows = env
    rng = np.random.default_rng(100 + delta_max)
    db = _db(env, delta_max=delta_max)
    model = Model(voc.nwords)
    live, next_key = [], 1000
    assert len(db.detect(RELOC, [bows[0]])[0]) == 0                   # empty database
    for step in range(260):
        op = rng.random()
        if op < 0.45 or len(live) < 4:
            base = bows[int(rng.integers(len(bows)))]
            bow = base if rng.random() < 0.15 else _variant(rng, base)   # exact copies: tied scores
            kf = KF(next_key, *bow)
            next_key += int(rng.integers(1, 5))
            db.add(kf.key, bow)
            model.add(kf)
            live.append(kf)
            _set_covis(db, rng, kf, live)
            if rng.random() < 0.3 and len(live) > 2:          # connections change as the map grows
                _set_covis(db, rng, live[int(rng.integers(len(live)))], live)
        elif op < 0.55:
            kf = live.pop(int(rng.integers(len(live))))
            db.erase(kf.key)
            model.erase(kf)
        elif op < 0.56:
            db.clear()
            model.clear()
            live = []
        elif op < 0.78:
            q = _variant(rng, bows[int(rng.integers(len(bows)))], 0.8)
            if rng.random() < 0.2:
                _check_score(db, model, RELOC, q)
            else:
                got = db.detect(RELOC, [q])[0]
                assert list(got) == _keys(model.detect_reloc(q)), step
        else:
            q = _variant(rng, bows[int(rng.integers(len(bows)))], 0.8)
            conn = set(rng.choice(live, min(len(live), int(rng.integers(0, 12))), replace=False)) if live else set()
            if rng.random() < 0.2:
                _check_score(db, model, LOOP, q, conn)
            else:
                ms = float(rng.choice([0.0, 0.01, 0.05]))
                got = db.detect(LOOP, [q], [[k.key for k in conn]], ms)[0]
                assert list(got) == _keys(model.detect_loop(q, conn, ms)), step
    info = db.info()
    assert info[0] == len(live)
    if delta_max:
        assert info[3] > 0                                     # the rebuild threshold was crossed mid-sequence


def test_edges(env):
    _, voc, bows = env
    db = _db(env, delta_max=8)
    model = Model(voc.nwords)
    rng = np.random.default_rng(7)
    kfs = [KF(i, *bows[i % 4]) for i in range(12)]            # ties: three copies of each of four vectors
    for k in kfs:
        db.add(k.key, k.bow)
        model.add(k)
    for k in kfs:
        k.covis = [kfs[(k.key + 1) % 12], kfs[(k.key + 5) % 12]]
        db.set_covis(k.key, [c.key for c in k.covis])
    # no shared word
    used = set(int(w) for k in kfs for w in k.bow[0])
    free = np.array(sorted(set(range(voc.nwords)) - used)[:20], np.uint32)
    q = (free, np.full(len(free), 1.0 / len(free)))
    assert len(db.detect(RELOC, [q])[0]) == 0 and model.detect_reloc(q) == []
    # every candidate connected
    q = _variant(rng, bows[1], 0.9)
    got = db.detect(LOOP, [q], [[k.key for k in kfs]], 0.0)[0]
    assert len(got) == 0 and model.detect_loop(q, set(kfs), 0.0) == []
    # query after erase, tied scores
    for e in (kfs[1], kfs[6]):
        db.erase(e.key)
        model.erase(e)
    for b in range(4):
        q = _variant(rng, bows[b], 0.9)
        _check_score(db, model, RELOC, q)
        assert list(db.detect(RELOC, [q])[0]) == _keys(model.detect_reloc(q))
        assert list(db.detect(LOOP, [q], [[]], 0.0)[0]) == _keys(model.detect_loop(q, set(), 0.0))
    # a 4000-word query
    w = np.sort(rng.choice(voc.nwords, 4000, replace=False)).astype(np.uint32)
    v = rng.random(4000)
    q = (w, v / v.sum())
    _check_score(db, model, RELOC, q)
    assert list(db.detect(LOOP, [q], [[]], 0.0)[0]) == _keys(model.detect_loop(q, set(), 0.0))


def _detect_device(db, mode, qs, excluded=None, min_score=0.0, cap=4096):
    from hiprt import DevBuf
    B = len(qs)
    arrs = db.pack(mode, qs, excluded)
    bufs = [DevBuf.from_numpy(a) for a in arrs]
    off, keys = DevBuf((B + 1) * 4), DevBuf(cap * 8)
    try:
        db.detect_device(mode, B, *[b.ptr.value for b in bufs], min_score, off.ptr.value, keys.ptr.value, cap)
        o = off.to_numpy(np.int32, B + 1)
        assert o[B] <= cap
        k = keys.to_numpy(np.uint64, max(int(o[B]), 1))
        return [k[o[b]:o[b + 1]] for b in range(B)]
    finally:
        for b in bufs + [off, keys]:
            b.free()


def test_batch_equals_sequential_calls_stale_scores_included(env):
    _, voc, bows = env
    rng = np.random.default_rng(11)
    db = _db(env, delta_max=32)
    model = Model(voc.nwords)
    live = []
    for i in range(150):
        kf = KF(i, *_variant(rng, bows[i % len(bows)], 0.6))
        db.add(kf.key, kf.bow)
        model.add(kf)
        live.append(kf)
    for kf in live:
        _set_covis(db, rng, kf, live)
    for B in (1, 7, 64):
        qs = [_variant(rng, bows[int(rng.integers(len(bows)))], 0.5) for _ in range(B)]
        got = db.detect(RELOC, qs)
        want = [_keys(model.detect_reloc(q)) for q in qs]
        assert [list(g) for g in got] == want
        qs = [_variant(rng, bows[int(rng.integers(len(bows)))], 0.5) for _ in range(B)]
        conn = [set(rng.choice(live, 5, replace=False)) for _ in range(B)]
        got = _detect_device(db, LOOP, qs, [[k.key for k in c] for c in conn], 0.01)
        assert [list(g) for g in got] == [_keys(model.detect_loop(q, c, 0.01)) for q, c in zip(qs, conn)]
    qs = [_variant(rng, bows[int(rng.integers(len(bows)))], 0.5) for _ in range(32)]
    got = _detect_device(db, RELOC, qs)
    assert [list(g) for g in got] == [_keys(model.detect_reloc(q)) for q in qs]


def test_many_key_frames(env):
    _, voc, bows = env
    rng = np.random.default_rng(13)
    N = 65536
    db = _db(env, max_kfs=N, delta_max=4096)
    model = Model(voc.nwords)
    live = []
    for i in range(N):
        b = bows[i % len(bows)]
        sel = np.sort(rng.choice(len(b[0]), 24, replace=False))
        v = b[1][sel] / b[1][sel].sum()
        kf = KF(i, b[0][sel], v)
        db.add(kf.key, (b[0][sel], v))
        model.add(kf)
        live.append(kf)
        if i in (4095, 4096, 4097, 20000):
            q = _variant(rng, bows[i % len(bows)], 0.5)
            assert list(db.detect(RELOC, [q])[0]) == _keys(model.detect_reloc(q))
    for kf in live[::97]:
        _set_covis(db, rng, kf, live[:500])
    for _ in range(3):
        q = _variant(rng, bows[int(rng.integers(len(bows)))], 0.3)
        _check_score(db, model, RELOC, q)
        assert list(db.detect(RELOC, [q])[0]) == _keys(model.detect_reloc(q))
        assert list(db.detect(LOOP, [q], [[1, 2, 3]], 0.0)[0]) == _keys(model.detect_loop(q, set(live[1:4]), 0.0))


def test_limits_return_errors(env):
    from orbhip.capi import OrbHipError
    _, voc, bows = env
    db = _db(env, max_kfs=4)
    with pytest.raises(OrbHipError):
        db.add(1, (np.arange(8193, dtype=np.uint32), np.ones(8193)))          # > 8192 words
    with pytest.raises(OrbHipError):
        db.add(1, (np.array([5, 3], np.uint32), np.ones(2)))                  # not ascending
    with pytest.raises(OrbHipError):
        db.add(1, (np.array([voc.nwords], np.uint32), np.ones(1)))           # beyond the vocabulary
    for k in range(4):
        db.add(k, bows[k])
    with pytest.raises(OrbHipError):
        db.add(0, bows[0])                                                    # already present
    with pytest.raises(OrbHipError):
        db.add(9, bows[0])                                                    # full
    with pytest.raises(OrbHipError):
        db.detect(RELOC, [(np.arange(8193, dtype=np.uint32), np.ones(8193))])
    with pytest.raises(OrbHipError):
        db.detect(RELOC, [bows[0]] * 1025)


def test_overflowing_reloc_batch_changes_nothing(env):
    """A reloc batch whose candidates do not fit fails without committing its scores as stale scores: the same batch again
    with room for them gives exactly what B sequential calls give (near-identical key frames: many tied candidates)."""
    from orbhip.capi import OrbHipError
    _, voc, bows = env
    rng = np.random.default_rng(17)
    db = _db(env, delta_max=64)
    model = Model(voc.nwords)
    live = []
    for i in range(240):
        kf = KF(i, *_variant(rng, bows[i % 6], 0.9))
        db.add(kf.key, kf.bow)
        model.add(kf)
        live.append(kf)
    for kf in live:
        _set_covis(db, rng, kf, live)
    for rnd in range(3):
        qs = [_variant(rng, bows[int(rng.integers(6))], 0.4) for _ in range(24)]
        got = db.detect(RELOC, qs, cap=1)                            # fails once, then the retry
        assert [list(g) for g in got] == [_keys(model.detect_reloc(q)) for q in qs], rnd
        qs = [_variant(rng, bows[int(rng.integers(6))], 0.4) for _ in range(24)]
        with pytest.raises(OrbHipError):
            _detect_device(db, RELOC, qs, cap=1)                    # the device entry point: same rule
        got = _detect_device(db, RELOC, qs)
        assert [list(g) for g in got] == [_keys(model.detect_reloc(q)) for q in qs], rnd


def test_device_entry_point_rejects_a_shifted_qoff(env):
    from hiprt import DevBuf
    from orbhip.capi import OrbHipError
    _, voc, bows = env
    db = _db(env)
    db.add(1, bows[0])
    qoff, qw, qv, xoff, xk = db.pack(RELOC, [bows[0]])
    qoff = qoff + 5                                                   # qoff[0] != 0
    bufs = [DevBuf.from_numpy(a) for a in (qoff, qw, qv, xoff, xk)]
    off, keys = DevBuf(8), DevBuf(64)
    try:
        with pytest.raises(OrbHipError):
            db.detect_device(RELOC, 1, *[b.ptr.value for b in bufs], 0.0, off.ptr.value, keys.ptr.value, 8)
    finally:
        for b in bufs + [off, keys]:
            b.free()
    assert list(db.detect(RELOC, [bows[0]])[0]) == [1]


def test_phase_times(env):
    _, voc, bows = env
    db = _db(env)
    for i in range(40):
        db.add(i, bows[i % len(bows)])
    db.set_timing(True)
    db.detect(LOOP, bows[:8], [[]] * 8, 0.0)
    ms = db.phase_times()
    assert (ms >= 0).all() and ms[0] > 0 and ms[5] > 0
