"""orbhip_pnp_score[_device] / orbhip_sim3_score[_device] on the GPU against the independent model (tests/ransac_model.py): counts,
record indices, results and flag bytes equal.  No tolerance anywhere.  The host forms write into poisoned buffers that are longer
than needed; what the call does not own must come back as it was."""
import numpy as np
import pytest

import ransac_model as M
import ransac_scenes as scenes

pytestmark = pytest.mark.gpu
f32, f64, i32 = np.float32, np.float64, np.int32
POISON = 0xAB
POISON32 = int(np.frombuffer(bytes([POISON] * 4), i32)[0])
EYE_RT = np.r_[np.eye(3).ravel(), np.zeros(3)]
EYE_T = np.tile(np.eye(4, dtype=f32)[:3].ravel(), 2)


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(500, max_w=320, max_h=240)
    yield e
    e.close()


def _pnp(ex, P3Dw, P2D, max_err, cam, Rt, min_inliers, best_in=0, R=8):
    """The host form into poisoned, over-long buffers -> the model's dict layout."""
    from orbhip import ransac
    N, Mh = len(np.asarray(max_err).ravel()), len(np.asarray(Rt).reshape(-1, 12))
    counts = np.full(Mh + 3, POISON32, i32)
    res = np.zeros(2, ransac.PNP_RESULT)
    res.view(np.uint8)[:] = POISON
    idx, cnt = np.full(R + 2, POISON32, i32), np.full(R + 2, POISON32, i32)
    flags = np.full(R * N + 16, POISON, np.uint8)
    ransac.pnp_score(ex, P3Dw, P2D, max_err, cam, Rt, min_inliers, best_in, R, out=(counts, res, idx, cnt, flags))
    n = min(int(res[0]["n_records"]), R)
    assert (counts[Mh:] == POISON32).all() and (res[1:].view(np.uint8) == POISON).all()
    assert (idx[n:] == POISON32).all() and (cnt[n:] == POISON32).all() and (flags[n * N:] == POISON).all()
    return dict(counts=counts[:Mh], n_records=int(res[0]["n_records"]), best_out=int(res[0]["best_out"]), rec_idx=idx[:n].tolist(),
                rec_cnt=cnt[:n].tolist(), rec_flags=flags[:n * N].reshape(n, N))


def _sim3(ex, X1, X2, p1, p2, e1, e2, K1, K2, T, min_inliers, best_in=0):
    from orbhip import ransac
    N, Mh = len(np.asarray(e1).ravel()), len(np.asarray(T).reshape(-1, 24))
    counts = np.full(Mh + 3, POISON32, i32)
    res = np.zeros(2, ransac.SIM3_RESULT)
    res.view(np.uint8)[:] = POISON
    flags = np.full(N + 16, POISON, np.uint8)
    ransac.sim3_score(ex, X1, X2, p1, p2, e1, e2, K1, K2, T, min_inliers, best_in, out=(counts, res, flags))
    assert (counts[Mh:] == POISON32).all() and (res[1:].view(np.uint8) == POISON).all() and (flags[N:] == POISON).all()
    r = res[0]
    return dict(counts=counts[:Mh], winner=int(r["winner"]), ninliers=int(r["ninliers"]), best_it=int(r["best_it"]),
                best_out=int(r["best_out"]), win_flags=flags[:N])


def _same(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), k


PNP_KEYS = ("counts", "n_records", "best_out", "rec_idx", "rec_cnt", "rec_flags")
SIM3_KEYS = ("counts", "winner", "ninliers", "best_it", "best_out", "win_flags")
_MODEL = {}


def _want(kind, N):
    """The model's flags of the N-point scene's 300 hypotheses: computed once, shared by the six M of the shape test."""
    if (kind, N) not in _MODEL:
        s = scenes.pnp(N, 300, seed=100 + N) if kind == "pnp" else scenes.sim3(N, 300, seed=200 + N)
        e = M.pnp_evaluate(*scenes.pnp_args(s), 0) if kind == "pnp" else M.sim3_evaluate(*scenes.sim3_args(s), 10 ** 6)
        e["flags"].setflags(write=False)
        _MODEL[(kind, N)] = (s, e["flags"])
    return _MODEL[(kind, N)]


# hypotheses taken from both ends of the scene's 300, so that every M sees good and useless ones
def _pick(Mh):
    return np.r_[np.arange((Mh + 1) // 2), np.arange(300 - Mh // 2, 300)]


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("Mh", [1, 7, 8, 9, 64, 300])
def test_shapes_against_the_model(ex, N, Mh):
    sel = _pick(Mh)
    s, flags = _want("pnp", N)
    counts = flags[sel].sum(1).astype(i32)
    mi = N // 4
    n, best, idx, cnt = M.pnp_select(counts, mi, 0, 8)
    got = _pnp(ex, s["P3Dw"], s["P2D"], s["max_err"], s["cam"], s["Rt"][sel], mi)
    _same(got, dict(counts=counts, n_records=n, best_out=best, rec_idx=idx, rec_cnt=cnt, rec_flags=flags[sel][idx].reshape(len(idx), N)), PNP_KEYS)
    if N >= 63:
        assert n >= 1 and counts.max() > N // 2
    s, flags = _want("sim3", N)
    counts = flags[sel].sum(1).astype(i32)
    for mi in (N // 4, N):                                                    # a winner (from N = 63 on), and none
        w, nin, it, best = M.sim3_select(counts, mi, 0)
        got = _sim3(ex, *scenes.sim3_args(s)[:8], s["T"][sel], mi)
        _same(got, dict(counts=counts, winner=w, ninliers=nin, best_it=it, best_out=best,
                        win_flags=flags[sel][w] if w >= 0 else np.zeros(N, np.uint8)), SIM3_KEYS)
        assert (w >= 0) == (N >= 63 and mi < N)


def test_guard_scene(ex):
    """tests/test_ransac_model.py shows that on these scenes a float division for invZc, a float gemm or a float dot product flips
    flags of hypothesis 0: equal flags here mean the device rounds where the contract says."""
    alt = (np.arange(257) % 2 == 0).astype(np.uint8)
    s = scenes.pnp_guard()
    got = _pnp(ex, *scenes.pnp_args(s), 0, R=9)
    want = M.pnp_evaluate(*scenes.pnp_args(s), 0, R=9)
    _same(got, want, PNP_KEYS)
    assert got["rec_idx"][0] == 0 and np.array_equal(got["rec_flags"][0], alt)
    s = scenes.sim3_guard()
    got = _sim3(ex, *scenes.sim3_args(s), 0)
    want = M.sim3_evaluate(*scenes.sim3_args(s), 0)
    _same(got, want, SIM3_KEYS)
    assert got["winner"] == 0 and np.array_equal(got["win_flags"], alt)


def test_threshold_and_depth_edges(ex):
    cam = (400.0, 400.0, 320.0, 240.0)
    uc, vc = f32(320), f32(240)
    # R = I, t = 0, X = (0, 0, 1), pixel (uc + 2, vc): error2 == 4 exactly
    X = np.array([[0, 0, 1]] * 2, f32)
    uv = np.array([[uc + 2, vc]] * 2, f32)
    me = np.array([4.0, np.nextafter(f32(4), f32(5))], f32)                   # == max_err fails, the next float passes
    got = _pnp(ex, X, uv, me, cam, [EYE_RT], 0)
    assert got["counts"].tolist() == [1] and got["rec_flags"].tolist() == [[0, 1]]
    # Z = 0: invZc = inf, error2 inf or NaN -> no inlier, whatever max_err; the neighbour point is unaffected
    X = np.array([[0, 0, 0], [1, 1, 0], [0, 0, 1]], f32)
    uv = np.array([[uc, vc]] * 3, f32)
    me = np.array([np.inf, np.inf, 1.0], f32)
    got = _pnp(ex, X, uv, me, cam, [EYE_RT], 0)
    _same(got, M.pnp_evaluate(X, uv, me, cam, [EYE_RT], 0), PNP_KEYS)
    assert got["rec_flags"].tolist() == [[0, 0, 1]]
    # behind the camera with a matching reprojection: an inlier (there is no test on the sign of the depth)
    X = np.array([[0.5, -0.25, -2.0]], f32)
    uv = np.array([[320 + 400 * 0.5 / -2.0, 240 + 400 * -0.25 / -2.0]], f32)
    got = _pnp(ex, X, uv, np.array([1.0], f32), cam, [EYE_RT], 0)
    assert got["counts"].tolist() == [1] and got["rec_flags"].tolist() == [[1]]
    # the same three for Sim3: X2 = X1, T = I, K1 = K2; pixel displaced by 2: err == 4
    K = (400.0, 400.0, 320.0, 240.0)
    X = np.array([[0, 0, 1]] * 2, f32)
    p = np.array([[uc, vc]] * 2, f32)
    p_off = np.array([[uc + 2, vc]] * 2, f32)
    me = np.array([4.0, np.nextafter(f32(4), f32(5))], f32)
    big = np.full(2, 100.0, f32)
    assert _sim3(ex, X, X, p_off, p, me, big, K, K, [EYE_T], 0)["win_flags"].tolist() == [0, 1]      # err1 on the edge
    assert _sim3(ex, X, X, p, p_off, big, me, K, K, [EYE_T], 0)["win_flags"].tolist() == [0, 1]      # err2 on the edge
    X0 = np.array([[0, 0, 0], [0, 0, 1]], f32)
    got = _sim3(ex, X0, X0, p, p, np.full(2, np.inf, f32), np.full(2, np.inf, f32), K, K, [EYE_T], 0)
    assert got["win_flags"].tolist() == [0, 1] and got["counts"].tolist() == [1]
    Xb = np.array([[0.5, -0.25, -2.0]], f32)
    pb = np.array([[320 + 400 * 0.5 / -2.0, 240 + 400 * -0.25 / -2.0]], f32)
    assert _sim3(ex, Xb, Xb, pb, pb, np.ones(1, f32), np.ones(1, f32), K, K, [EYE_T], 0)["win_flags"].tolist() == [1]


def test_nan_hypothesis_leaves_its_neighbours_alone(ex):
    s = scenes.pnp(257, 12, seed=7)
    clean = M.pnp_evaluate(*scenes.pnp_args(s), 0)["counts"]
    Rt = s["Rt"].copy()
    Rt[5, 4] = np.nan
    Rt[4, 11] = np.inf
    got = _pnp(ex, s["P3Dw"], s["P2D"], s["max_err"], s["cam"], Rt, 0, R=12)
    _same(got, M.pnp_evaluate(s["P3Dw"], s["P2D"], s["max_err"], s["cam"], Rt, 0, R=12), PNP_KEYS)
    keep = np.ones(12, bool)
    keep[[4, 5]] = False
    assert np.array_equal(got["counts"][keep], clean[keep]) and clean[5] > 0 and got["counts"][5] == 0
    s = scenes.sim3(257, 12, seed=8)
    clean = M.sim3_evaluate(*scenes.sim3_args(s), 10 ** 6)["counts"]
    T = s["T"].copy()
    T[3, 2], T[6, 20] = np.nan, np.nan
    keep[:] = True
    keep[[3, 6]] = False
    got = _sim3(ex, *scenes.sim3_args(s)[:8], T, 10 ** 6)
    _same(got, M.sim3_evaluate(*scenes.sim3_args(s)[:8], T, 10 ** 6), SIM3_KEYS)
    assert np.array_equal(got["counts"][keep], clean[keep]) and got["counts"][3] == 0 and got["counts"][6] == 0 and clean[3] > 0 < clean[6]


def _pnp_with_counts(N, want_counts):
    """A PnP problem whose hypotheses have exactly the wanted counts: N points on the optical axis at depths 1 .. N, every pixel the
    principal point, max_err 1.  The identity moved sideways by t_x displaces the point at depth z by fu * t_x / z pixels, so
    t_x = (N - c + 0.5) / fu leaves exactly the c deepest points within 1 px."""
    cam = (400.0, 400.0, 320.0, 240.0)
    X = np.zeros((N, 3), f32)
    X[:, 2] = np.arange(1, N + 1)
    uv = np.tile(np.array([320, 240], f32), (N, 1))
    me = np.ones(N, f32)
    Rt = np.tile(EYE_RT, (len(want_counts), 1))
    for h, c in enumerate(want_counts):
        Rt[h, 9] = (N - c + 0.5) / 400.0
    return X, uv, me, cam, Rt


def test_pnp_selection_edges(ex):
    want_counts = [3, 5, 5, 4, 7, 7, 9, 12, 11, 20]
    a = _pnp_with_counts(32, want_counts)
    got = _pnp(ex, *a, 5)
    assert got["counts"].tolist() == want_counts                               # the construction gives the counts it promises
    # count == min_inliers is a record (h = 1), an equal later count is not (h = 2, h = 5)
    assert got["rec_idx"] == [1, 4, 6, 7, 9] and got["rec_cnt"] == [5, 7, 9, 12, 20] and got["n_records"] == 5 and got["best_out"] == 20
    _same(got, M.pnp_evaluate(*a, 5), PNP_KEYS)
    # n_records > R: the lists are cut, the total is not
    got = _pnp(ex, *a, 5, R=2)
    assert got["n_records"] == 5 and got["rec_idx"] == [1, 4] and got["best_out"] == 20 and got["rec_flags"].sum(1).tolist() == [5, 7]
    _same(got, M.pnp_evaluate(*a, 5, R=2), PNP_KEYS)
    # best_in carried: nothing at or below it is a record
    got = _pnp(ex, *a, 5, best_in=9)
    assert got["rec_idx"] == [7, 9] and got["n_records"] == 2
    # N < min_inliers: no error, no record; M == 0: none, best_out = best_in
    got = _pnp(ex, *a, 33, best_in=2)
    assert got["n_records"] == 0 and got["best_out"] == 2 and got["counts"].tolist() == want_counts
    got = _pnp(ex, a[0], a[1], a[2], a[3], np.zeros((0, 12)), 5, best_in=4)
    assert got["n_records"] == 0 and got["best_out"] == 4 and len(got["counts"]) == 0


def _sim3_with_counts(N, want_counts):
    """The same construction for Sim3: X1 = X2 on the optical axis at depths 1 .. N, T12 = T21 = identity but for a sideways shift in
    T12 that leaves exactly the c deepest points within 1 px in image 1; image 2 always agrees."""
    K = (400.0, 400.0, 320.0, 240.0)
    X = np.zeros((N, 3), f32)
    X[:, 2] = np.arange(1, N + 1)
    p = np.tile(np.array([320, 240], f32), (N, 1))
    T = np.tile(EYE_T, (len(want_counts), 1))
    for h, c in enumerate(want_counts):
        T[h, 3] = (N - c + 0.5) / 400.0
    return X, X, p, p, np.ones(N, f32), np.full(N, 10.0, f32), K, K, T


def test_sim3_selection_edges(ex):
    want_counts = [3, 5, 5, 4, 7, 6, 12, 30, 31]
    a = _sim3_with_counts(32, want_counts)
    got = _sim3(ex, *a, 7)
    assert got["counts"].tolist() == want_counts
    # 7 == min_inliers is no winner (h = 4); 12 is (h = 6); nothing after it is looked at: best_out is 12, not 31
    assert (got["winner"], got["ninliers"], got["best_it"], got["best_out"]) == (6, 12, 6, 12) and got["win_flags"].sum() == 12
    _same(got, M.sim3_evaluate(*a, 7), SIM3_KEYS)
    # equal counts move best_it to the later hypothesis
    got = _sim3(ex, *a[:8], a[8][:4], 7)
    assert (got["winner"], got["ninliers"], got["best_it"], got["best_out"]) == (-1, 0, 2, 5) and not got["win_flags"].any()
    # no hypothesis reaches best_in: best_it = -1
    got = _sim3(ex, *a[:8], a[8][:4], 7, best_in=6)
    assert (got["winner"], got["best_it"], got["best_out"]) == (-1, -1, 6)
    # N < min_inliers is no error; M == 0: none, best_out = best_in, flags 0
    got = _sim3(ex, *a, 40)
    assert got["winner"] == -1 and got["best_it"] == 8 and got["best_out"] == 31
    got = _sim3(ex, *a[:8], np.zeros((0, 24), f32), 7, best_in=3)
    assert (got["winner"], got["ninliers"], got["best_it"], got["best_out"]) == (-1, 0, -1, 3) and not got["win_flags"].any()


def test_carry_one_call_of_300_against_60_calls_of_5(ex):
    s = scenes.pnp(257, 300, seed=3)
    Rt = s["Rt"][::-1].copy()                                                  # reversed: the counts rise, records keep coming
    a = scenes.pnp_args(s)[:4]
    whole = _pnp(ex, *a, Rt, 40, R=300)
    best, n, idx, cnt, rows = 0, 0, [], [], []
    for h0 in range(0, 300, 5):
        g = _pnp(ex, *a, Rt[h0:h0 + 5], 40, best_in=best, R=5)
        best, n = g["best_out"], n + g["n_records"]
        idx, cnt = idx + [h0 + v for v in g["rec_idx"]], cnt + g["rec_cnt"]
        rows += list(g["rec_flags"])
    assert whole["n_records"] > 5 and (n, best, idx, cnt) == (whole["n_records"], whole["best_out"], whole["rec_idx"], whole["rec_cnt"])
    assert np.array_equal(np.array(rows), whole["rec_flags"])
    _same(whole, M.pnp_evaluate(*a, Rt, 40, R=300), PNP_KEYS)
    s = scenes.sim3(257, 300, seed=4)
    T = s["T"][::-1].copy()
    a = scenes.sim3_args(s)[:8]
    whole = _sim3(ex, *a, T, 120)
    best, best_it, g, h0 = 0, -1, None, 0
    for h0 in range(0, 300, 5):
        g = _sim3(ex, *a, T[h0:h0 + 5], 120, best_in=best)
        best = g["best_out"]
        if g["best_it"] >= 0:
            best_it = h0 + g["best_it"]
        if g["winner"] >= 0:
            break
    assert whole["winner"] > 5 and (h0 + g["winner"], g["ninliers"], best_it, best) == (whole["winner"], whole["ninliers"], whole["best_it"], whole["best_out"])
    assert np.array_equal(g["win_flags"], whole["win_flags"])
    _same(whole, M.sim3_evaluate(*a, T, 120), SIM3_KEYS)


NS_DEVICE = [0, 3, 64, 257, 1000]


def test_device_forms_equal_host_calls(ex):
    """B = 5 problems of N = 0, 3, 64, 257 and 1000 points in one call, with different min_inliers and best_in, against five
    host-form calls."""
    import hiprt
    from orbhip import ransac
    B, Mh, R = len(NS_DEVICE), 20, 3
    off = np.r_[0, np.cumsum(NS_DEVICE)].astype(i32)
    tot = int(off[-1])
    mi, bi = np.array([0, 1, 16, 60, 250], i32), np.array([0, 0, 20, 0, 300], i32)
    ps = [scenes.pnp(N, Mh, seed=40 + b) for b, N in enumerate(NS_DEVICE)]
    cat = lambda k, src: np.concatenate([np.asarray(s[k], f32) for s in src])      # along the points; the N = 0 scene adds nothing
    bufs = [hiprt.DevBuf.from_numpy(cat(k, ps)) for k in ("P3Dw", "P2D", "max_err")] + [hiprt.DevBuf.from_numpy(np.stack([s["Rt"] for s in ps]))]
    outs = [hiprt.DevBuf.from_numpy(np.full(n, POISON, np.uint8)) for n in (B * Mh * 4 + 8, B * 8 + 8, B * R * 4 + 8, B * R * 4 + 8, R * tot + 8)]
    ransac.pnp_score_device(ex, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, off, scenes.CAM, bufs[3].ptr, Mh, mi, bi, R, *[o.ptr for o in outs])
    ex.sync()
    counts, res = outs[0].to_numpy(i32, (B, Mh)), outs[1].to_numpy(ransac.PNP_RESULT, (B,))
    idx, cnt, flags = outs[2].to_numpy(i32, (B, R)), outs[3].to_numpy(i32, (B, R)), outs[4].to_numpy(np.uint8, (R * tot + 8,))
    assert (flags[R * tot:] == POISON).all() and (outs[0].to_numpy(np.uint8, (B * Mh * 4 + 8,))[-8:] == POISON).all()
    some = 0
    for b, s in enumerate(ps):
        N = NS_DEVICE[b]
        h = _pnp(ex, *scenes.pnp_args(s), int(mi[b]), int(bi[b]), R=R)
        n = min(h["n_records"], R)
        assert np.array_equal(counts[b], h["counts"]) and (int(res[b]["n_records"]), int(res[b]["best_out"])) == (h["n_records"], h["best_out"])
        assert idx[b, :n].tolist() == h["rec_idx"] and cnt[b, :n].tolist() == h["rec_cnt"] and (idx[b, n:] == POISON32).all()
        rows = flags[R * off[b]:R * off[b + 1]].reshape(R, N)
        assert np.array_equal(rows[:n], h["rec_flags"]) and (rows[n:] == POISON).all()
        some += n
    assert some >= 4
    for x in bufs + outs:
        x.free()

    ss = [scenes.sim3(N, Mh, seed=50 + b) for b, N in enumerate(NS_DEVICE)]
    keys = ("X3Dc1", "X3Dc2", "P1im1", "P2im2", "max_err1", "max_err2")
    bufs = [hiprt.DevBuf.from_numpy(cat(k, ss)) for k in keys] + [hiprt.DevBuf.from_numpy(np.stack([s["T"] for s in ss]))]
    outs = [hiprt.DevBuf.from_numpy(np.full(n, POISON, np.uint8)) for n in (B * Mh * 4 + 8, B * 16 + 8, tot + 8)]
    mi = np.array([0, 1, 16, 60, 2000], i32)
    ransac.sim3_score_device(ex, *[x.ptr for x in bufs[:6]], off, scenes.K1, scenes.K2, bufs[6].ptr, Mh, mi, bi, *[o.ptr for o in outs])
    ex.sync()
    counts, res, flags = outs[0].to_numpy(i32, (B, Mh)), outs[1].to_numpy(ransac.SIM3_RESULT, (B,)), outs[2].to_numpy(np.uint8, (tot + 8,))
    assert (flags[tot:] == POISON).all()
    for b, s in enumerate(ss):
        h = _sim3(ex, *scenes.sim3_args(s), int(mi[b]), int(bi[b]))
        assert np.array_equal(counts[b], h["counts"]) and res[b].tolist() == (h["winner"], h["ninliers"], h["best_it"], h["best_out"])
        assert np.array_equal(flags[off[b]:off[b + 1]], h["win_flags"])
    assert res["winner"][2] >= 0 and res["winner"][3] >= 0 and res["winner"][4] == -1
    for x in bufs + outs:
        x.free()


def test_errors_leave_outputs_untouched(ex):
    import hiprt
    from orbhip import capi, ransac
    from orbhip.capi import _p
    L = capi.load()
    s, t = scenes.pnp(8, 4, seed=7), scenes.sim3(8, 4, seed=7)
    X, uv, me, cam, Rt = [np.ascontiguousarray(a) for a in scenes.pnp_args(s)]
    ta = [np.ascontiguousarray(a, f32) for a in scenes.sim3_args(t)]

    def pnp(N=8, Mh=4, mi=2, R=2):
        outs = [np.full(64, POISON, np.uint8) for _ in range(5)]
        rc = L.orbhip_pnp_score(ex.handle, _p(X), _p(uv), _p(me), N, *cam, _p(Rt), Mh, mi, 0, R, *[_p(o) for o in outs])
        return rc, all((o == POISON).all() for o in outs)

    def sim3(N=8, Mh=4, mi=2):
        outs = [np.full(64, POISON, np.uint8) for _ in range(3)]
        rc = L.orbhip_sim3_score(ex.handle, *[_p(a) for a in ta[:6]], N, _p(ta[6]), _p(ta[7]), _p(ta[8]), Mh, mi, 0, *[_p(o) for o in outs])
        return rc, all((o == POISON).all() for o in outs)

    assert pnp() == (0, False) and sim3() == (0, False)
    for kw in (dict(N=-1), dict(Mh=-1), dict(Mh=65536), dict(R=0), dict(R=-3), dict(mi=-1)):
        rc, untouched = pnp(**kw)
        assert rc == -1 and untouched and capi.last_error(ex.handle), kw        # ORBHIP_E_ARG
    for kw in (dict(N=-1), dict(Mh=-1), dict(Mh=65536), dict(mi=-1)):
        rc, untouched = sim3(**kw)
        assert rc == -1 and untouched and capi.last_error(ex.handle), kw
    # the device forms: the same checks, and off, before anything is enqueued
    d = hiprt.DevBuf.from_numpy(np.full(1 << 16, POISON, np.uint8))
    k4 = np.array(scenes.K1, f32)
    ok_off, ok_mi = np.array([0, 3, 8], i32), np.array([1, 1], i32)

    def dev_pnp(off=ok_off, B=2, Mh=4, mi=ok_mi, R=2):
        return L.orbhip_pnp_score_device(ex.handle, d.ptr, d.ptr, d.ptr, _p(off), B, *cam, d.ptr, Mh, _p(mi), None, R, d.ptr, d.ptr, d.ptr, d.ptr,
                                         d.ptr)

    def dev(off=ok_off, B=2, Mh=4, mi=ok_mi):
        a = dev_pnp(off, B, Mh, mi)
        b = L.orbhip_sim3_score_device(ex.handle, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, _p(off), B, _p(k4), _p(k4), d.ptr, Mh, _p(mi), None,
                                       d.ptr, d.ptr, d.ptr)
        return a, b

    cases = [dict(off=np.array([0, 5, 3], i32)), dict(off=np.array([-1, 3, 8], i32)), dict(B=-1), dict(B=65536), dict(Mh=-1), dict(Mh=65536),
             dict(mi=np.array([1, -1], i32))]
    for kw in cases:
        if kw.get("B") == 65536:
            kw["off"], kw["mi"] = np.zeros(65537, i32), np.zeros(65536, i32)
        assert dev(**kw) == (-1, -1) and capi.last_error(ex.handle), kw
    assert dev_pnp(R=0) == -1 and dev_pnp(R=-1) == -1
    ex.sync()
    assert (d.to_numpy(np.uint8, (1 << 16,)) == POISON).all()
    d.free()
