"""The C++ drop-in ORB_SLAM2::LocalMapSearch (include/orbhip/LocalMap.h): against a mock of the entry points it calls (no device:
argument marshalling, the skip byte, member write-back, the F.mvpMapPoints rules), and on the device against the host restatement
of the reference's loop + the existing ORBmatcher::SearchByProjection on the same Frame / MapPoint objects
(tests/native_localmap/test_localmap_dropin.cpp), whose counts must also be the independent model's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_localmap")
f32 = np.float32


def _prog(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_localmap/%s is not built (run __graft_entry__.build())" % name
    return p


def test_class_against_a_mock_of_the_entry_points():
    out = subprocess.run([_prog("test_localmap_mock")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,th", [("640x480", 1.0), ("752x480", 3.0), ("1241x376_stereo", 5.0)])
def test_dropin_equals_the_reference_loop_on_the_same_objects(oracle, tmp_path, name, th):
    import localmap_model as M
    import localmap_scenes as scenes
    sc = scenes.make(oracle, name)
    rng = np.random.default_rng(3)
    skip = (rng.random(len(sc["keys"])) < 0.05).astype(np.uint8)
    # features that already hold a point: with observations (closed to the search), without (may be overwritten)
    occ_kind = np.where(sc["occupied"] != 0, 1, np.where(rng.random(len(sc["kps"])) < 0.05, 2, 0))
    path = str(tmp_path / "scene.bin")
    scenes.write_scene(path, sc, th, skip, occ_kind)
    out = subprocess.run([_prog("test_localmap_dropin"), path], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    store = M.Store(len(sc["keys"]))
    store.put(sc["keys"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["pdesc"], sc["flags"])
    rec, code, ntm, nm, match, q, qd = M.search_local_points(oracle, store, sc["cam"], th, sc["keys"], skip, sc["kps"], sc["desc"],
                                                             sc["gp"], 0.8, sc["u_right"], sc["occupied"])
    assert [int(x) for x in out.stdout.split()[1:3]] == [ntm, nm] and nm >= 100
