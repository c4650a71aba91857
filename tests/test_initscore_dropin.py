"""The C++ drop-in's initialiser scoring: ORB_SLAM2::InitializerScore on the device (tests/native_initscore/test_initscore_dropin.cpp)
against that program's own host restatement of the reference's loops -- it exits non-zero on any difference -- and, here, against
the independent model: SH, SF, the winning iterations, and the two vector<bool> in mvMatches12 order."""
import os
import struct
import subprocess

import numpy as np
import pytest

import initscore_model as M
import initscore_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "native_initscore", "test_initscore_dropin")
f32 = np.float32


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["planar", "general"])
def test_dropin_scores_equal_the_host_restatement_and_the_model(scene, tmp_path):
    assert os.path.exists(PROG), "tests/native_initscore/test_initscore_dropin is not built (run __graft_entry__.build())"
    k1, k2, m, Ht = scenes.planar(150, seed=31)
    kg, k2g, mg, Ft = scenes.general(150, seed=32)
    H21, H12 = scenes.homographies(Ht, 200)
    F21 = scenes.fundamentals(Ft, 200)
    if scene == "general":
        k1, k2, m = kg, k2g, mg
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4if", len(k1), len(k2), len(H21), len(F21), 1.0) + k1.tobytes() + k2.tobytes() + m.tobytes() +
                H21.tobytes() + H12.tobytes() + F21.tobytes())
    out = subprocess.run([PROG, src, dst], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    raw = open(dst, "rb").read()
    N, itH, itF = struct.unpack_from("<3i", raw)
    SH, SF = np.frombuffer(raw, f32, 2, 12)
    inH, inF = np.frombuffer(raw, np.uint8, N, 20), np.frombuffer(raw, np.uint8, N, 20 + N)
    assert len(raw) == 20 + 2 * N and N == 150
    want = M.evaluate(k1, k2, m, H21, H12, F21, 1.0)
    assert (itH, itF) == tuple(want["best"]["it"]) and (itH if scene == "planar" else itF) >= 0
    assert np.array_equal(np.array([SH, SF], f32).view(np.uint32), np.ascontiguousarray(want["best"]["score"]).view(np.uint32))
    # mvMatches12 order: the flags of the matched frame-1 features, compacted in index order
    assert np.array_equal(inH, want["inliers"][0][want["idx"]]) and np.array_equal(inF, want["inliers"][1][want["idx"]])
    assert inH.sum() == want["best"]["ninliers"][0] and inF.sum() == want["best"]["ninliers"][1]
    assert (inH.sum() if scene == "planar" else inF.sum()) > 100
