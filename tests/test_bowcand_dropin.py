"""ORB_SLAM2::LocalMapSearch::SearchByBoWCandidates (include/orbhip/LocalMap.h), both overloads, over a map of 30 key frames and
1200 points on mock KeyFrame / MapPoint / Frame objects with three rounds of map edits (tests/native_bowcand/test_bowcand.cpp):
against a host model of the entry point and per-candidate SearchByBoW plus the PnPsolver-constructor loop on a twin map (no device:
the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device, whose line of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_bowcand")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_bowcand/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    calls, device, host = [int(x) for x in line[0].split()[1:4]]
    assert calls > 15 and device > 0 and host > 0           # both ways ran: the call, and ORBmatcher::SearchByBoW for an unknown point
    return line[0]


def test_class_against_a_host_model_of_the_entry_point():
    _run("test_bowcand_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_bowcand_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_bowcand_dropin") == _run("test_bowcand_mock")
