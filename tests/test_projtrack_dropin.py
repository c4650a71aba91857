"""ORB_SLAM2::LocalMapSearch::SearchLastFrame / SearchKeyFramePoints (include/orbhip/LocalMap.h) over a sequence of frames on
mock Frame / KeyFrame / MapPoint objects, with temporal points, points turned bad and points erased with their slots re-used
(tests/native_projtrack/test_projtrack.cpp): against a host model of the entry points and the restated reference loops (no
device: the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device against ORBmatcher's two methods, whose
line of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_projtrack")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_projtrack/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    frames, calls, matches = [int(x) for x in out.stdout.split()[1:4]]
    assert frames == 8 and calls >= 30 and matches > 3000
    return out.stdout


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_projtrack_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_projtrack_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_orbmatcher_on_the_same_objects():
    assert _run("test_projtrack_dropin") == _run("test_projtrack_mock")
