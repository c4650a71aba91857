"""ORB_SLAM2::LocalMapSearch::SearchLoopPoints / SearchAndFuse (include/orbhip/LocalMap.h) over a small map on mock KeyFrame /
MapPoint objects (tests/native_loopfuse/test_loopfuse.cpp): against a host model of the three entry points and the reference's
sequential loops restated on the host (no device: the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device
against ORBmatcher::SearchByProjection(pKF, Scw, ...) and ORBmatcher::Fuse(pKF, Scw, ...) called per key frame, whose line of
output must be the mock program's.  The programs themselves assert that the resident state afterwards equals a fresh Put /
PutKeyFrame of every object and that the map differs when changed survivors are not searched again."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_loopfuse")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_loopfuse/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    points, matches, bad = [int(x) for x in line[0].split()[1:4]]
    assert points >= 200 and matches >= 20 and bad >= 100
    return line[0], out.stdout


def test_class_against_a_host_model_of_the_entry_points():
    line, out = _run("test_loopfuse_mock")
    # the program asserts them, and says so: what the scene must hold for the sequencing rules to be tested at all
    note = re.search(r"changed and active later (\d+), of them with another best feature (\d+); held later (\d+); added then held (\d+)", out)
    assert note and int(note.group(1)) >= 10 and int(note.group(2)) >= 1 and int(note.group(3)) >= 10 and int(note.group(4)) >= 1


def test_class_against_the_host_model_under_sanitizers():
    _run("test_loopfuse_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_the_orbmatcher_path_on_the_same_objects():
    assert _run("test_loopfuse_dropin")[0] == _run("test_loopfuse_mock")[0]
