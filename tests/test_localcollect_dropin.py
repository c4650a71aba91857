"""ORB_SLAM2::LocalMapSearch::UpdateLocalMap / TrackLocalPoints (include/orbhip/LocalMap.h) against a host restatement of
Tracking::UpdateLocalMap on the same mock KeyFrame / MapPoint objects, over a map that grows, fuses, replaces and culls points and
loses key frames between frames (tests/native_localcollect/test_localcollect.cpp): against a host model of the entry points (no
device: the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_localcollect")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_localcollect/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    frames, kfs, pts, largest = [int(x) for x in out.stdout.split()[1:5]]
    assert frames == 120 and kfs > 80 and largest > 300
    return out.stdout


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_localcollect_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_localcollect_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_reference_loops_on_the_same_objects():
    assert _run("test_localcollect_dropin") == _run("test_localcollect_mock")
