"""ORB_SLAM2::LocalMapSearch::KeyFrameCulling (include/orbhip/LocalMap.h) over a map of 30 key frames and 1200 points on mock
KeyFrame / MapPoint objects, monocular and stereo, with a skip functor that reads what the previous cull changed, and two hand-built
scenes in which one batch of counts at the start gives the wrong answer (tests/native_cull/test_cull.cpp): against a host model of
the entry points and the sequential loop of tests/native_cull/ref_cull.h on a twin map (no device: the class's bookkeeping, also
under AddressSanitizer / UBSan), and on the device, whose line of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_cull")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_cull/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    culled, device, host = [int(x) for x in line[0].split()[1:4]]
    assert culled > 10 and device > 100 and host > 3           # both ways ran: the call, and the loop for an unknown point
    return line[0]


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_cull_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_cull_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_cull_dropin") == _run("test_cull_mock")
