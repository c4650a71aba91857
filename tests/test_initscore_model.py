"""The independent model of the initialiser's hypothesis scoring (tests/initscore_model.py) against answers worked out by hand,
and the guard that keeps the GPU order test honest: on its scene a sum in another order must give other bits."""
import numpy as np

import initscore_model as M
import initscore_scenes as scenes

f32 = np.float32
EYE = np.eye(3, dtype=f32).ravel()


def _one_pair(p1, p2):
    return scenes.keypoints([p1]), scenes.keypoints([p2]), np.array([0], np.int32)


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def test_homography_known_answers():
    th = f32(5.991)
    k1, k2, m = _one_pair((10, 20), (11, 20))                  # displaced by (1, 0): each chiSquare is 1
    r = M.evaluate(k1, k2, m, [EYE], [EYE], None, 1.0)
    want = f32(f32(th - f32(1)) + f32(th - f32(1)))
    assert _bits(r["scores"])[0] == _bits(want) and r["inliers"].tolist() == [[1], [0]]
    assert r["best"][0].tolist() == (want, 0, 1) and r["best"][1].tolist() == (0.0, -1, 0)
    k1, k2, m = _one_pair((10, 20), (13, 20))                  # displaced by (3, 0): 9 > 5.991 twice
    r = M.evaluate(k1, k2, m, [EYE], [EYE], None, 1.0)
    assert _bits(r["scores"])[0] == 0 and r["inliers"].tolist() == [[0], [0]] and r["best"][0].tolist() == (0.0, -1, 0)


def test_fundamental_known_answers():
    th = f32(5.991)
    k1, k2, m = _one_pair((10, 20), (50, 21))                  # vertical offset 1: each chiSquare is 1 <= 3.841, scored with 5.991
    r = M.evaluate(k1, k2, m, None, None, [scenes.F_DEGENERATE], 1.0)
    want = f32(f32(th - f32(1)) + f32(th - f32(1)))
    assert _bits(r["scores"])[0] == _bits(want) and r["inliers"].tolist() == [[0], [1]]
    assert r["best"][1].tolist() == (want, 0, 1) and r["best"][0].tolist() == (0.0, -1, 0)
    k1, k2, m = _one_pair((10, 20), (50, 23))                  # vertical offset 3: 9 > 3.841 twice
    r = M.evaluate(k1, k2, m, None, None, [scenes.F_DEGENERATE], 1.0)
    assert _bits(r["scores"])[0] == 0 and r["inliers"].tolist() == [[0], [0]] and r["best"][1].tolist() == (0.0, -1, 0)
    k1, k2, m = _one_pair((10, 20), (50, 22))                  # offset 2: 4 > 3.841 although 4 < 5.991 -- the two thresholds differ
    r = M.evaluate(k1, k2, m, None, None, [scenes.F_DEGENERATE], 1.0)
    assert _bits(r["scores"])[0] == 0 and r["best"][1]["it"] == -1


def test_inv_sigma_square_and_the_nan_rule():
    assert M.inv_sigma_square(1.0) == f32(1.0) and M.inv_sigma_square(2.0) == f32(0.25)
    assert M.inv_sigma_square(0.903) == f32(1.0 / float(f32(0.903) * f32(0.903)))
    # an all-zero F: 0 / 0 is NaN, NaN > th is false, the term is added and the score is NaN; a NaN never beats 0
    k1, k2, m = _one_pair((10, 20), (50, 21))
    r = M.evaluate(k1, k2, m, None, None, [np.zeros((3, 3), f32), scenes.F_DEGENERATE], 1.0)
    assert np.isnan(r["scores"][0]) and r["best"][1]["it"] == 1 and r["inliers"][1].tolist() == [1]
    assert M.winner(np.array([np.nan, 0.0, -1.0], f32)) == (f32(0.0), -1)
    assert M.winner(np.array([1.0, 2.0, 2.0, np.nan], f32)) == (f32(2.0), 1)          # the first of the largest


def test_scatter_to_frame1_indices_and_unmatched_entries():
    k1, k2, m, Ht = scenes.planar(33)
    assert len(k1) == 33 + 9 and (m >= 0).sum() == 33 and m[0] == -1 and m[-1] == -1 and (m[10:30] == -1).any()
    H21, H12 = scenes.homographies(Ht, 5)
    r = M.evaluate(k1, k2, m, H21, H12, None, 1.0)
    assert r["best"][0]["it"] >= 0 and r["best"][0]["ninliers"] == r["inliers"][0].sum() > 20
    assert not r["inliers"][0][m < 0].any() and not r["inliers"][1].any()


def test_order_guard_sequential_sum_differs_from_numpy_sum():
    """The GPU order test compares scores by bit pattern on this scene.  That only shows the order if another order gives other
    bits: np.sum (pairwise) of the same included terms must differ from the sequential sum for at least a quarter of the hypotheses."""
    k1, k2, m, Ht = scenes.planar(33)
    H21, H12 = scenes.homographies(Ht, 200)
    idx, u1, v1, u2, v2 = M.pairs(k1, k2, m)
    differ = 0
    for a, b in zip(H21, H12):
        c1, c2 = M.chi_h(a, b, u1, v1, u2, v2, f32(1.0))
        vals, skipped, _ = M.terms(c1, c2, M.TH_H)
        seq = M.sequential_sum(vals, skipped)[0]
        other = np.sum(vals[~skipped], dtype=f32)
        differ += _bits(seq) != _bits(other)
    print("sequential sum != np.sum for %d of 200 hypotheses" % differ)
    assert differ >= 50
