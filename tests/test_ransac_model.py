"""The independent model of the RANSAC inlier checks (tests/ransac_model.py) against the reference's loops restated in C++
(tests/native_ransac/ransac_host_loops, g++ -O2 -ffp-contract=off), the guard that keeps the GPU comparison honest -- on its scene
another rounding of the same formulas must flip a flag -- and the chunk invariance of the selection rules.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac_model as M
import ransac_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "native_ransac", "ransac_host_loops")
i32 = np.int32


def _host_loops(kind, s, min_inliers, best_in, tmp_path):
    assert os.path.exists(PROG), "tests/native_ransac/ransac_host_loops is not built (run __graft_entry__.build())"
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(scenes.scene_bytes(kind, s, min_inliers, best_in))
    out = subprocess.run([PROG, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    raw = open(dst, "rb").read()
    k, N, Mh = struct.unpack_from("<3i", raw)
    counts = np.frombuffer(raw, i32, Mh, 12)
    flags = np.frombuffer(raw, np.uint8, Mh * N, 12 + 4 * Mh).reshape(Mh, N)
    tail = np.frombuffer(raw, i32, offset=12 + 4 * Mh + Mh * N)
    return counts, flags, tail


@pytest.mark.parametrize("N,Mh,min_inliers,best_in", [(257, 64, 10, 0), (65, 300, 30, 0), (1000, 9, 300, 500), (1, 7, 0, 0), (0, 5, 0, 0)])
def test_model_equals_the_restated_host_loops(N, Mh, min_inliers, best_in, tmp_path):
    s = scenes.pnp(N, Mh, seed=10 + N)
    counts, flags, tail = _host_loops("pnp", s, min_inliers, best_in, tmp_path)
    want = M.pnp_evaluate(*scenes.pnp_args(s), min_inliers, best_in, R=None)
    assert np.array_equal(flags, want["flags"]) and np.array_equal(counts, want["counts"])
    n = want["n_records"]
    assert tail.tolist() == [n, want["best_out"]] + want["rec_idx"] + want["rec_cnt"]
    if N >= 65:
        assert counts.max() > N // 2 and counts.min() < N // 8 and len(set(counts.tolist())) < Mh      # spread, and ties
    s = scenes.sim3(N, Mh, seed=20 + N)
    counts, flags, tail = _host_loops("sim3", s, min_inliers, best_in, tmp_path)
    want = M.sim3_evaluate(*scenes.sim3_args(s), min_inliers, best_in)
    assert np.array_equal(flags, want["flags"]) and np.array_equal(counts, want["counts"])
    assert tail.tolist() == [want["winner"], want["ninliers"], want["best_it"], want["best_out"]]
    if N >= 65:
        assert counts.max() > N // 2 and counts.min() < N // 8 and len(set(counts.tolist())) < Mh


def test_guard_scene_tells_the_roundings_apart(tmp_path):
    """max_err[i] is the model's own error of point i under hypothesis 0, one ulp up (even i) or down (odd i).  The pinned
    arithmetic gives exactly the alternating flags; invZc as one float division flips a PnP flag; a float accumulator in Project's
    gemm, or in the dot product, flips a Sim3 flag.  The GPU tests compare the device with the model on these same scenes."""
    alt = (np.arange(257) % 2 == 0).astype(np.uint8)
    s = scenes.pnp_guard()
    P3Dw, P2D, max_err, cam, Rt = scenes.pnp_args(s)
    assert np.array_equal(M.pnp_flags(Rt[0], P3Dw, P2D, max_err, cam), alt)
    flipped = int((M.pnp_flags(Rt[0], P3Dw, P2D, max_err, cam, "float_div") != alt).sum())
    print("PnP guard: invZc as a float division flips %d of 257 flags" % flipped)
    assert flipped >= 1
    assert np.array_equal(_host_loops("pnp", s, 0, 0, tmp_path)[1][0], alt)                  # the C++ restatement is on the model's side
    s = scenes.sim3_guard()
    a = scenes.sim3_args(s)
    pts, T = a[:8], a[8]
    assert np.array_equal(M.sim3_flags(T[0], *pts), alt)
    for variant in ("float_gemm", "float_dot"):
        flipped = int((M.sim3_flags(T[0], *pts, variant=variant) != alt).sum())
        print("Sim3 guard: %s flips %d of 257 flags" % (variant, flipped))
        assert flipped >= 1
    assert np.array_equal(_host_loops("sim3", s, 0, 0, tmp_path)[1][0], alt)


def _chained_pnp(counts, min_inliers, chunk, R):
    best, n, idx, cnt = 0, 0, [], []
    for h0 in range(0, len(counts), chunk):
        k, best, i, c = M.pnp_select(counts[h0:h0 + chunk], min_inliers, best, R)
        n, idx, cnt = n + k, idx + [h0 + v for v in i], cnt + c
    return n, best, idx, cnt


def _chained_sim3(counts, min_inliers, chunk):
    best, best_it = 0, -1
    for h0 in range(0, len(counts), chunk):
        w, n, it, best = M.sim3_select(counts[h0:h0 + chunk], min_inliers, best)
        if it >= 0:
            best_it = h0 + it
        if w >= 0:
            return h0 + w, n, best_it, best
    return -1, 0, best_it, best


@pytest.mark.parametrize("min_inliers", [0, 40, 120, 1000])
def test_selection_is_chunk_invariant(min_inliers):
    """300 hypotheses at once against 60 chunks of 5 with best_out fed back as best_in and the indices offset."""
    s = scenes.pnp(257, 300, seed=3)
    counts = M.pnp_evaluate(*scenes.pnp_args(s), 0)["counts"][::-1].copy()        # reversed: the counts rise, so records keep coming
    assert M.pnp_select(counts, min_inliers, 0, None) == _chained_pnp(counts, min_inliers, 5, None)
    if min_inliers == 40:
        assert M.pnp_select(counts, min_inliers, 0, None)[0] > 5
    s = scenes.sim3(257, 300, seed=4)
    counts = M.sim3_evaluate(*scenes.sim3_args(s), 10 ** 6)["counts"][::-1].copy()
    assert M.sim3_select(counts, min_inliers, 0) == _chained_sim3(counts, min_inliers, 5)
    if min_inliers == 120:
        assert M.sim3_select(counts, min_inliers, 0)[0] > 5                        # the winner is not in the first chunk


def test_selection_rules_by_hand():
    assert M.pnp_select([3, 5, 5, 4, 7], 5) == (2, 7, [1, 4], [5, 7])              # == min_inliers is a record, an equal later count is not
    assert M.pnp_select([3, 5, 5, 4, 7], 5, best_in=5) == (1, 7, [4], [7])
    assert M.pnp_select([6, 7, 8, 9], 0, R=2) == (4, 9, [0, 1], [6, 7])            # the lists are cut, the total is not
    assert M.pnp_select([], 3, best_in=4) == (0, 4, [], [])
    assert M.sim3_select([5, 5, 4], 5) == (-1, 0, 1, 5)                            # == min_inliers is no winner; equal counts move best_it on
    assert M.sim3_select([5, 6, 9], 5) == (1, 6, 1, 6)                             # nothing after the winner is looked at
    assert M.sim3_select([2, 3], 5, best_in=4) == (-1, 0, -1, 4)
    assert M.sim3_select([0, 0], 0) == (-1, 0, 1, 0)                               # N == 0: 0 >= 0 moves best_it, 0 > 0 never wins
    assert M.sim3_select([], 0, best_in=7) == (-1, 0, -1, 7)
