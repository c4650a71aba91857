"""ORB_SLAM2::LocalMapSearch::BuildLocalBA / BuildBAProblem (include/orbhip/LocalMap.h) over a map of 12 key frames and 1500 points
on mock KeyFrame / MapPoint objects, with a bad point and a culled key frame that its neighbours still list
(tests/native_baproblem/test_baproblem.cpp): the five vectors and the stamps against the reference's three loops
(tests/native_baproblem/ref_ba.h) on a twin map, and the `false` path for a failing entry point and for a key frame without a row.
Against a host model of the entry points (no device: the class's bookkeeping, also under AddressSanitizer / UBSan as a stand-alone
program), and on the device, whose line of output must be the mock program's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_baproblem")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_baproblem/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    problems, edges = [int(x) for x in line[0].split()[1:3]]
    assert problems == 13 and edges > 30000                    # eleven local problems, the window and the global one
    return line[0]


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_baproblem_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_baproblem_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_mock_programs_line():
    assert _run("test_baproblem_dropin") == _run("test_baproblem_mock")
