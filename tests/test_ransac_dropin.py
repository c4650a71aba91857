"""The C++ drop-in's RANSAC scoring: ORB_SLAM2::RansacScore on the device (tests/native_ransac/test_ransac_dropin.cpp) against that
program's own host restatement of the reference's loops -- it exits non-zero on any difference -- and, here, against the
independent model: every count, the records / the winner and their inlier flags."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ransac_model as M
import ransac_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "native_ransac", "test_ransac_dropin")
i32 = np.int32


def _run(kind, s, min_inliers, best_in, tmp_path):
    assert os.path.exists(PROG), "tests/native_ransac/test_ransac_dropin is not built (run __graft_entry__.build())"
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(scenes.scene_bytes(kind, s, min_inliers, best_in))
    out = subprocess.run([PROG, src, dst], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.startswith("ok " + kind), out.stdout + out.stderr
    return open(dst, "rb").read()


@pytest.mark.gpu
def test_pnp_dropin_equals_the_host_restatement_and_the_model(tmp_path):
    s = scenes.pnp(300, 100, seed=31)
    s["Rt"] = s["Rt"][::-1].copy()                                            # rising counts: several records
    raw = _run("pnp", s, 30, 10, tmp_path)
    kind, N, Mh, nrec, best, kept = struct.unpack_from("<6i", raw)
    want = M.pnp_evaluate(*scenes.pnp_args(s), 30, 10, R=64)
    assert (kind, N, Mh, nrec, best) == (0, 300, 100, want["n_records"], want["best_out"]) and kept == len(want["rec_idx"]) > 3
    assert len(raw) == 24 + 4 * Mh + 8 * kept + kept * N
    assert np.array_equal(np.frombuffer(raw, i32, Mh, 24), want["counts"])
    assert np.frombuffer(raw, i32, kept, 24 + 4 * Mh).tolist() == want["rec_idx"]
    assert np.frombuffer(raw, i32, kept, 24 + 4 * Mh + 4 * kept).tolist() == want["rec_cnt"]
    assert np.array_equal(np.frombuffer(raw, np.uint8, kept * N, 24 + 4 * Mh + 8 * kept).reshape(kept, N), want["rec_flags"])


@pytest.mark.gpu
@pytest.mark.parametrize("min_inliers", [100, 10 ** 6])
def test_sim3_dropin_equals_the_host_restatement_and_the_model(min_inliers, tmp_path):
    s = scenes.sim3(300, 100, seed=32)
    s["T"] = s["T"][::-1].copy()
    raw = _run("sim3", s, min_inliers, 10, tmp_path)
    head = struct.unpack_from("<7i", raw)
    want = M.sim3_evaluate(*scenes.sim3_args(s), min_inliers, 10)
    assert head == (1, 300, 100, want["winner"], want["ninliers"], want["best_it"], want["best_out"])
    assert (want["winner"] > 3) == (min_inliers == 100) and want["best_it"] >= 0
    assert len(raw) == 28 + 4 * 100 + 300
    assert np.array_equal(np.frombuffer(raw, i32, 100, 28), want["counts"])
    assert np.array_equal(np.frombuffer(raw, np.uint8, 300, 428), want["win_flags"])
