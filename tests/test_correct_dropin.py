"""ORB_SLAM2::LocalMapSearch::CorrectLoopPoints and ApplyGlobalBA (include/orbhip/LocalMap.h) over a map of 30 key frames and 1200
points on mock KeyFrame / MapPoint objects, against the reference's loops written out on a twin map
(tests/native_correct/test_correct.cpp, ref_correct.h): on a host model of the two entry points (no device: the class's bookkeeping and
the rank rule against the sequence, also under AddressSanitizer / UBSan), and on the device, whose line of output must be the mock
program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_correct")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_correct/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    loop, gba, device, host = [int(x) for x in line[0].split()[1:5]]
    assert loop >= 600 and gba >= 800 and device > 0 and host == 7   # both ways ran in both calls
    return line[0]


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_correct_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_correct_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_correct_dropin") == _run("test_correct_mock")
