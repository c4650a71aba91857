"""orbhip_init_score[_device] on the GPU against the independent model (tests/initscore_model.py): scores by bit pattern, records
and inlier bytes equal.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import initscore_model as M
import initscore_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EYE = np.eye(3, dtype=f32).ravel()
POISON = 0xAB


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(500, max_w=320, max_h=240)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_scores(got, want):
    """NaN by class, everything else by bit pattern."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _run(ex, k1, k2, m, H21, H12, F21, sigma=1.0):
    """The host form into poisoned buffers that are longer than needed; the tails must come back as they were."""
    from orbhip import initscore
    n1 = len(k1)
    nhyp = (0 if H21 is None else len(H21)) + (0 if F21 is None else len(F21))
    scores = np.full(nhyp + 3, np.float32(-7.5), f32)
    best = np.zeros(3, initscore.BEST_DTYPE)
    best.view(np.uint8)[:] = POISON
    inl = np.full(2 * n1 + 16, POISON, np.uint8)
    initscore.init_score(ex, k1, k2, m, H21, H12, F21, sigma, out=(scores, best, inl))
    assert (scores[nhyp:] == np.float32(-7.5)).all() and (best[2:].view(np.uint8) == POISON).all() and (inl[2 * n1:] == POISON).all()
    return scores[:nhyp], best[:2], inl[:2 * n1].reshape(2, n1)


def _check(ex, k1, k2, m, H21, H12, F21, sigma=1.0):
    got = _run(ex, k1, k2, m, H21, H12, F21, sigma)
    want = M.evaluate(k1, k2, m, H21, H12, F21, sigma)
    assert _same_scores(got[0], want["scores"])
    assert _same_scores(got[1]["score"], want["best"]["score"])
    assert np.array_equal(got[1]["it"], want["best"]["it"]) and np.array_equal(got[1]["ninliers"], want["best"]["ninliers"])
    assert np.array_equal(got[2], want["inliers"])
    return got, want


@pytest.mark.parametrize("N", [0, 1, 7, 8, 63, 64, 65, 257, 1000])
def test_shapes_against_the_model(ex, N):
    kp, k2p, mp, Ht = scenes.planar(N, seed=100 + N)
    kg, k2g, mg, Ft = scenes.general(N, seed=200 + N)
    assert len(kp) > N and (mp >= 0).sum() == N and mp[0] == -1 and mp[-1] == -1      # n1 > N: unmatched at the front, the end ...
    assert N < 2 or (mp[4:-4] == -1).any()                                             # ... and in the middle
    H21, H12 = scenes.homographies(Ht, 200)
    F21 = scenes.fundamentals(Ft, 200)
    for nH, nF in [(0, 1), (1, 0), (1, 1), (63, 65), (64, 64), (200, 200)]:
        a = (H21[:nH], H12[:nH]) if nH else (None, None)
        b = F21[:nF] if nF else None
        (_, gb, _), _ = _check(ex, kp, k2p, mp, a[0], a[1], b)
        (_, gg, _), _ = _check(ex, kg, k2g, mg, a[0], a[1], b)
        if N >= 63 and nH >= 63:
            assert gb[0]["it"] >= 0 and gb[0]["ninliers"] > N // 2                     # the scenes do have winners: the planar one
            assert gg[1]["it"] >= 0 and gg[1]["ninliers"] > N // 2                     # by H, the general one by F


def test_sum_order_on_the_guard_scene(ex):
    """tests/test_initscore_model.py shows that on this scene np.sum's order gives other bits for more than a quarter of the
    hypotheses: equal bits here mean the terms were added in match order."""
    k1, k2, m, Ht = scenes.planar(33)
    H21, H12 = scenes.homographies(Ht, 200)
    got, want = _check(ex, k1, k2, m, H21, H12, None)
    assert np.array_equal(_bits(got[0]), _bits(want["scores"])) and (got[0] > 0).sum() > 150


def _edge(chi_of, start, target):
    """(below, at, above): `start` must give chiSquare == target exactly; the nearest floats on either side of it whose chiSquare
    is smaller / larger."""
    assert chi_of(start) == target, "the edge input does not reach equality"
    lo = hi = f32(start)
    for _ in range(64):
        lo = np.nextafter(lo, f32(0))
        if chi_of(lo) < target:
            break
    for _ in range(64):
        hi = np.nextafter(hi, f32(np.inf))
        if chi_of(hi) > target:
            break
    assert chi_of(lo) < target < chi_of(hi)
    return lo, f32(start), hi


def test_homography_threshold_edges(ex):
    """Identity, sigma = 1, the pair (0, 0) -> (2, dy) with fl(4 + fl(dy * dy)) == 5.991f exactly.  The dy is looked for here, among
    the floats around sqrt(1.991), and the set-up fails if there is none (0x3FB49C91 is one)."""
    chi_of = lambda d: f32(f32(4) + f32(f32(d) * f32(d)))
    near = int(f32(np.sqrt(1.991)).view(np.uint32))
    hits = [d for d in np.arange(near - 64, near + 64, dtype=np.uint32).view(f32) if chi_of(d) == M.TH_H]
    assert hits, "no dy lands on the threshold"
    below, at, above = _edge(chi_of, hits[0], M.TH_H)
    far = np.array([1, 0, 100, 0, 1, 0, 0, 0, 1], f32)                                  # carries every point 100 px away: its term is out
    for dy, inside in ((below, True), (at, True), (above, False)):
        for p1, p2 in (((0, 0), (2, dy)), ((2, dy), (0, 0))):                           # and the pair swapped
            # a second, perfect pair gives hypothesis 0 a positive score whatever the edge pair does: it wins, and its flags show
            k1, k2, m = scenes.keypoints([p1, (50, 60)]), scenes.keypoints([p2, (50, 60)]), np.array([0, 1], np.int32)
            # both terms on the edge | term 1 alone (image 1, through H12) | term 2 alone (image 2, through H21)
            H21 = np.stack([EYE, far, EYE])
            H12 = np.stack([EYE, EYE, far])
            got, want = _check(ex, k1, k2, m, H21, H12, None)
            c1, c2 = want["chi"][0][1][0][0], want["chi"][0][2][1][0]
            assert (c1 <= M.TH_H) == inside and (c2 <= M.TH_H) == inside and (c1 == M.TH_H) == (dy == at) == (c2 == M.TH_H)
            assert got[1][0]["it"] == 0 and got[2][0].tolist() == [int(inside), 1]
            both = f32(f32(M.TH_H - c1) + f32(M.TH_H - c2)) if inside else f32(0)
            assert _bits(got[0][0]) == _bits(f32(f32(both + M.TH_H) + M.TH_H))           # ... + (5.991 - 0) + (5.991 - 0), in order


def test_fundamental_threshold_edges(ex):
    sigma, dy0 = f32(0.903), f32(1.7697418)
    inv = M.inv_sigma_square(sigma)
    below, at, above = _edge(lambda d: f32(f32(f32(d) * f32(d)) * inv), dy0, M.TH_F)
    for dy, inside in ((below, True), (at, True), (above, False)):
        for p1, p2 in (((0, 0), (5, dy)), ((5, dy), (0, 0))):
            k1, k2, m = scenes.keypoints([p1, (10, 30)]), scenes.keypoints([p2, (70, 30)]), np.array([0, 1], np.int32)   # (and a perfect pair)
            got, want = _check(ex, k1, k2, m, None, None, scenes.F_DEGENERATE.reshape(1, 9), sigma)
            c1, c2 = want["chi"][1][0][0][0], want["chi"][1][0][1][0]
            assert (c1 <= M.TH_F) == inside and (c2 <= M.TH_F) == inside and (c1 == M.TH_F) == (dy == at) == (c2 == M.TH_F)
            assert got[1][1]["it"] == 0 and got[2][1].tolist() == [int(inside), 1]


def test_winner_rule(ex):
    k1, k2, m, Ht = scenes.planar(65, seed=5)
    H21, H12 = scenes.homographies(Ht, 200)
    sc = M.evaluate(k1, k2, m, H21, H12, None, 1.0)["scores"]
    top = int(np.argmax(sc))
    # the best hypothesis three times: the first copy wins
    a, b = H21.copy(), H12.copy()
    a[top], b[top] = H21[199], H12[199]
    for i in (3, 17, 150):
        a[i], b[i] = H21[top], H12[top]
    got, _ = _check(ex, k1, k2, m, a, b, a)                     # (the same matrices as F hypotheses: an arbitrary second model)
    assert got[1][0]["it"] == 3 and _bits(got[0][3]) == _bits(got[0][17]) == _bits(got[0][150])
    # the best hypothesis last
    a, b = H21.copy(), H12.copy()
    a[[top, 199]], b[[top, 199]] = a[[199, top]], b[[199, top]]
    got, _ = _check(ex, k1, k2, m, a, b, None)
    assert got[1][0]["it"] == 199
    # every hypothesis scores 0: nobody wins
    far = np.tile(np.array([1, 0, 500, 0, 1, 0, 0, 0, 1], f32), (70, 1))
    got, _ = _check(ex, k1, k2, m, far, far, far)
    assert (got[0] == 0).all() and got[1]["it"].tolist() == [-1, -1] and _bits(got[1]["score"]).tolist() == [0, 0]
    assert not got[2].any() and got[1]["ninliers"].tolist() == [0, 0]


def test_non_finite_hypotheses_among_good_ones(ex):
    k1, k2, m, Ht = scenes.planar(65, seed=6)
    first = int(np.nonzero(m >= 0)[0][0])
    k1["x"][first], k1["y"][first] = 4.0, 2.0                                            # exactly representable: the rows below hit 0
    H21, H12 = scenes.homographies(Ht, 12)
    F21 = scenes.fundamentals(scenes.general(65, seed=6)[3], 12)
    clean = M.evaluate(k1, k2, m, H21, H12, F21, 1.0)["scores"]
    H21b, F21b = H21.copy(), F21.copy()
    H21b[4, 6:9] = (0.5, 0.0, -2.0)                                                      # 0.5 * 4 + 0 * 2 - 2 = 0: w = 1 / 0 = inf, the term is out
    H21b[7] = (1, 0, -4, 0, 1, -2, 0.5, 0, -2)                                           # and 0 * inf on top: a NaN term, which is added
    F21b[5] = 0                                                                          # 0 / 0 in every term
    got, want = _check(ex, k1, k2, m, H21b, H12, F21b)
    assert np.isnan(want["scores"][7]) and np.isnan(want["scores"][12 + 5]) and np.isfinite(want["scores"][4])
    assert got[1][0]["it"] not in (4, 7) and got[1][1]["it"] != 5 and got[1][0]["it"] >= 0
    keep = np.ones(24, bool)
    keep[[4, 7, 12 + 5]] = False
    assert np.array_equal(_bits(got[0])[keep], _bits(clean)[keep])                       # the neighbours' scores are unaffected


def test_errors_leave_outputs_untouched(ex):
    from orbhip import capi, initscore
    k1, k2, m, Ht = scenes.planar(8, seed=7)
    H21, H12 = scenes.homographies(Ht, 4)
    L = capi.load()

    def call(n1=len(k1), n2=len(k2), match=m, nH=4, nF=4, sigma=1.0):
        scores = np.full(16, np.float32(-7.5), f32)
        best = np.zeros(2, initscore.BEST_DTYPE)
        best.view(np.uint8)[:] = POISON
        inl = np.full(2 * len(k1), POISON, np.uint8)
        mm = np.ascontiguousarray(match, np.int32)
        rc = L.orbhip_init_score(ex.handle, capi._p(k1), n1, capi._p(k2), n2, capi._p(mm), capi._p(H21), capi._p(H12), nH, capi._p(H21),
                                 nF, f32(sigma), capi._p(scores), capi._p(best), capi._p(inl))
        untouched = (scores == np.float32(-7.5)).all() and (best.view(np.uint8) == POISON).all() and (inl == POISON).all()
        return rc, untouched

    assert call() == (0, False)
    bad = m.copy()
    bad[np.nonzero(m >= 0)[0][2]] = len(k2)
    for kw in (dict(n1=-1), dict(n2=-1), dict(nH=-1), dict(nF=-2), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=np.inf),
               dict(sigma=np.nan), dict(nH=65535, nF=1), dict(match=bad)):
        rc, untouched = call(**kw)
        assert rc == -1 and untouched and capi.last_error(ex.handle), kw                 # ORBHIP_E_ARG
    # the device form: the same checks before anything is enqueued
    import hiprt
    d = hiprt.DevBuf(4096)
    args = lambda B=1, nH=1, nF=1, sigma=1.0: (ex.handle, d.ptr, d.ptr, 8, d.ptr, d.ptr, 8, B, d.ptr, d.ptr, d.ptr, nH, d.ptr, nF,
                                                f32(sigma), d.ptr, d.ptr, d.ptr)
    for kw in (dict(B=0), dict(B=65536), dict(nH=-1), dict(nF=-1), dict(sigma=0.0), dict(sigma=np.nan), dict(nH=65535, nF=1)):
        assert L.orbhip_init_score_device(*args(**kw)) == -1 and capi.last_error(ex.handle), kw
    assert not d.to_numpy(np.uint8, (4096,)).any()
    d.free()


def _device_problem_set(problems, nH, nF, hyps):
    """B problems -> the [B][cap] arrays of the device form."""
    from orbhip.capi import KP_DTYPE
    B = len(problems)
    cap1, cap2 = max(len(p[0]) for p in problems) + 5, max(len(p[1]) for p in problems) + 3
    K1, K2 = np.zeros((B, cap1), KP_DTYPE), np.zeros((B, cap2), KP_DTYPE)
    m = np.full((B, cap1), 123456, np.int32)                                             # (rows beyond cnt1 are never read)
    for b, (k1, k2, mm) in enumerate(problems):
        K1[b, :len(k1)], K2[b, :len(k2)], m[b, :len(k1)] = k1, k2, mm
    c1 = np.array([len(p[0]) for p in problems], np.int32)
    c2 = np.array([len(p[1]) for p in problems], np.int32)
    return K1, K2, m, c1, c2, cap1, cap2


def test_batched_device_form_equals_host_calls(ex):
    import hiprt
    from orbhip import initscore
    nH, nF = 20, 13
    problems, hyps = [], []
    for b, N in enumerate([40, 0, 200, 7, 65]):
        k1, k2, m, Ht = scenes.planar(N, seed=300 + b, extra1=0 if b == 1 else 4 + b, extra2=2 * b)
        if b == 3:
            m[np.nonzero(m >= 0)[0][1]] = len(k2) + 2                                    # outside [0, cnt2): unmatched in the device form
        problems.append((k1, k2, m))
        H21, H12 = scenes.homographies(Ht, nH, seed=400 + b)
        hyps.append((H21, H12, scenes.fundamentals(scenes.general(9, seed=b)[3], nF, seed=500 + b)))
    assert len(problems[1][0]) == 0                                                      # cnt1 = 0
    K1, K2, m, c1, c2, cap1, cap2 = _device_problem_set(problems, nH, nF, hyps)
    B = len(problems)
    bufs = [hiprt.DevBuf.from_numpy(a) for a in (K1, c1, K2, c2, m, np.stack([h[0] for h in hyps]), np.stack([h[1] for h in hyps]),
                                                 np.stack([h[2] for h in hyps]))]
    d_scores = hiprt.DevBuf.from_numpy(np.full((B, nH + nF), -7.5, f32))
    d_best = hiprt.DevBuf.from_numpy(np.full(B * 2 * 12, POISON, np.uint8))
    d_inl = hiprt.DevBuf.from_numpy(np.full((B, 2, cap1), POISON, np.uint8))
    initscore.init_score_device(ex, bufs[0].ptr, bufs[1].ptr, cap1, bufs[2].ptr, bufs[3].ptr, cap2, B, bufs[4].ptr, bufs[5].ptr,
                                bufs[6].ptr, nH, bufs[7].ptr, nF, 1.0, d_scores.ptr, d_best.ptr, d_inl.ptr)
    ex.sync()
    scores = d_scores.to_numpy(f32, (B, nH + nF))
    best = d_best.to_numpy(initscore.BEST_DTYPE, (B, 2))
    inl = d_inl.to_numpy(np.uint8, (B, 2, cap1))
    for b, (k1, k2, mm) in enumerate(problems):
        host_m = np.where(mm >= len(k2), -1, mm).astype(np.int32)                        # (the host form refuses such an entry)
        hs, hb, hi = _run(ex, k1, k2, host_m, hyps[b][0], hyps[b][1], hyps[b][2])
        assert np.array_equal(_bits(scores[b]), _bits(hs)) and best[b].tobytes() == hb.tobytes()
        assert np.array_equal(inl[b, :, :len(k1)], hi) and (inl[b, :, len(k1):] == POISON).all()
        want = M.evaluate(k1, k2, mm, hyps[b][0], hyps[b][1], hyps[b][2], 1.0, n2=len(k2))
        assert _same_scores(scores[b], want["scores"]) and np.array_equal(inl[b, :, :len(k1)], want["inliers"])
    assert best[1]["it"].tolist() == [-1, -1] and (scores[1] == 0).all()
    for x in bufs + [d_scores, d_best, d_inl]:
        x.free()


def _dlt_homography(p1, p2):
    A = []
    for (x, y), (u, v) in zip(p1, p2):
        A.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
    h = np.linalg.svd(np.asarray(A, np.float64))[2][-1].reshape(3, 3)
    return h / h[2, 2]


def test_chained_behind_search_for_initialization_device(ex):
    """Golden frame pair: grid -> orbhip_search_for_initialization_device -> orbhip_init_score_device on one stream; the matches
    never visit the host in between."""
    import hiprt
    from orbhip import capi, initscore
    from orbhip.capi import check
    g = np.load(os.path.join(GOLD, "init_search_376x241.npz"))
    k1, d1, k2, d2, gp = g["kps1"], g["desc1"], g["kps2"], g["desc2"], [float(v) for v in g["grid"]]
    want_m = g["matches12"]
    idx = np.nonzero(want_m >= 0)[0]
    assert len(idx) > 60
    # hypotheses from the golden matches, known before the device runs: a least-squares homography and perturbations of it
    p1 = np.stack([k1["x"][idx], k1["y"][idx]], 1).astype(np.float64)
    p2 = np.stack([k2["x"][want_m[idx]], k2["y"][want_m[idx]]], 1).astype(np.float64)
    H21, H12 = scenes.homographies(_dlt_homography(p1, p2), 40, seed=21)
    F21 = scenes.fundamentals(scenes.F_DEGENERATE.astype(np.float64) + 1e-9, 24, seed=22)
    n1, n2, L = len(k1), len(k2), capi.load()
    b = [hiprt.DevBuf.from_numpy(a) for a in (k1, d1, np.array([n1], np.int32), k2, d2, np.array([n2], np.int32), g["prev"], H21, H12, F21)]
    d_off, d_idx, d_m, d_nm = hiprt.DevBuf((64 * 48 + 1) * 4), hiprt.DevBuf(n2 * 4), hiprt.DevBuf(n1 * 4), hiprt.DevBuf(4)
    d_scores, d_best, d_inl = hiprt.DevBuf(64 * 4), hiprt.DevBuf(24), hiprt.DevBuf(2 * n1)
    check(L.orbhip_grid_build_device(ex.handle, b[3].ptr, b[5].ptr, n2, 1, gp[0], gp[1], gp[2], gp[3], d_off.ptr, d_idx.ptr), ex.handle, "grid")
    check(L.orbhip_search_for_initialization_device(ex.handle, b[0].ptr, b[1].ptr, b[2].ptr, n1, b[3].ptr, b[4].ptr, b[5].ptr, n2, 1,
                                                    gp[0], gp[1], gp[2], gp[3], d_off.ptr, d_idx.ptr, b[6].ptr, 30, 0.9, 1, d_m.ptr,
                                                    d_nm.ptr), ex.handle, "search_for_initialization_device")
    initscore.init_score_device(ex, b[0].ptr, b[2].ptr, n1, b[3].ptr, b[5].ptr, n2, 1, d_m.ptr, b[7].ptr, b[8].ptr, 40, b[9].ptr, 24, 1.0,
                                d_scores.ptr, d_best.ptr, d_inl.ptr)
    ex.sync()
    assert np.array_equal(d_m.to_numpy(np.int32, (n1,)), want_m)
    want = M.evaluate(k1, k2, want_m, H21, H12, F21, 1.0)
    assert _same_scores(d_scores.to_numpy(f32, (64,)), want["scores"])
    assert d_best.to_numpy(initscore.BEST_DTYPE, (2,)).tobytes() == want["best"].astype(initscore.BEST_DTYPE).tobytes()
    assert np.array_equal(d_inl.to_numpy(np.uint8, (2, n1)), want["inliers"])
    assert want["best"][0]["it"] >= 0 and want["best"][0]["ninliers"] > 30
    for x in b + [d_off, d_idx, d_m, d_nm, d_scores, d_best, d_inl]:
        x.free()
