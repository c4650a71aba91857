"""ORB_SLAM2::LocalMapSearch::FuseInTargets / FuseCandidates (include/orbhip/LocalMap.h) over a small map on mock KeyFrame /
MapPoint objects, three rounds of both passes with a Replace that changes a survivor's descriptor between two targets
(tests/native_fuse/test_fuse.cpp): against a host model of the entry points and the reference's sequential Fuse restated on the
host (no device: the class's bookkeeping, also under AddressSanitizer / UBSan), and on the device against ORBmatcher::Fuse called
per target, whose line of output must be the mock program's."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_fuse")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_fuse/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    line = [l for l in out.stdout.splitlines() if not l.startswith("#")]
    assert out.returncode == 0 and len(line) == 1 and line[0].startswith("ok "), out.stdout[-3000:] + out.stderr[-3000:]
    rounds, in_targets, candidates, bad = [int(x) for x in line[0].split()[1:5]]
    assert rounds == 3 and in_targets >= 1000 and candidates >= 100 and bad >= 100
    return line[0], out.stdout


def test_class_against_a_host_model_of_the_entry_points():
    line, out = _run("test_fuse_mock")
    # the program asserts it, and says so: points that survived a Replace in an early target and find another feature later
    note = re.search(r"changed and active later (\d+), of them with another best feature (\d+)", out)
    assert note and int(note.group(1)) >= 10 and int(note.group(2)) >= 1


def test_class_against_the_host_model_under_sanitizers():
    _run("test_fuse_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_orbmatcher_fuse_per_target_on_the_same_objects():
    assert _run("test_fuse_dropin")[0] == _run("test_fuse_mock")[0]
