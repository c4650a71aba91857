"""ORB_SLAM2::LocalMapSearch::UpdateConnections (include/orbhip/LocalMap.h) over a map of 40 key frames and 1500 points on mock
KeyFrame / MapPoint objects, three rounds of map edits between updates, single and batched, and a LoopConnections round
(tests/native_covis/test_covis.cpp): against a host model of the entry points and sequential KeyFrame::UpdateConnections of
slamlite.h on a twin map (no device: the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device, whose line
of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_covis")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_covis/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    updates, device, host = [int(x) for x in line[0].split()[1:4]]
    assert updates > 100 and device > 0 and host > 0           # both ways ran: the call, and the method for an unknown point
    return line[0]


def test_class_against_a_host_model_of_the_entry_point():
    _run("test_covis_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_covis_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_covis_dropin") == _run("test_covis_mock")
