"""ORB_SLAM2::LocalMapSearch::SearchBySim3 (include/orbhip/LocalMap.h) over the two sides of a loop on mock KeyFrame / MapPoint
objects (tests/native_sim3search/test_sim3search.cpp): against a host model of the entry point and the reference's loops restated on
the host (no device: the class's bookkeeping and its three -1 paths, also under AddressSanitizer / UBSan), and on the device against
ORBmatcher::SearchBySim3 on a twin map, whose line of output must be the mock program's.  The programs themselves assert that the
scene yields at least 20 agreed pairs and a one-sided match in each direction."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_sim3search")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_sim3search/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    agreed, one0, one1 = [int(x) for x in line[0].split()[1:4]]
    assert agreed >= 20 and one0 >= 1 and one1 >= 1
    return line[0], out.stdout


def test_class_against_a_host_model_of_the_entry_point():
    line, out = _run("test_sim3search_mock")
    note = re.search(r"features (\d+) / (\d+), points (\d+) \(bad (\d+)\), matched before (\d+)", out)
    assert note and int(note.group(1)) >= 200 and int(note.group(2)) >= 200 and int(note.group(1)) != int(note.group(2))
    assert int(note.group(3)) >= 300 and int(note.group(4)) >= 5 and int(note.group(5)) >= 5


def test_sim3search_mock_asan():
    _run("test_sim3search_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_orbmatcher_path_on_the_same_objects():
    assert _run("test_sim3search_dropin")[0] == _run("test_sim3search_mock")[0]
