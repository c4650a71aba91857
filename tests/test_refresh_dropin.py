"""ORB_SLAM2::LocalMapSearch::RefreshPoints (include/orbhip/LocalMap.h) over a map of 40 key frames and 1500 points on mock KeyFrame
/ MapPoint objects, three rounds of map edits between refreshes (tests/native_refresh/test_refresh.cpp): against a host model of the
entry points and the per-point methods of slamlite.h (no device: the class's bookkeeping, also under AddressSanitizer / UBSan), and
on the device, whose line of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_refresh")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_refresh/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    refreshes, device, host = [int(x) for x in line[0].split()[1:4]]
    assert refreshes == 7 and device > 0 and host > 0          # both ways ran: the call, and the fallback beyond the set limit
    return line[0]


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_refresh_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_refresh_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_refresh_dropin") == _run("test_refresh_mock")
