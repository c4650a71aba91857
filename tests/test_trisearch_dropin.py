"""ORB_SLAM2::TriangulationSearch (include/orbhip/TriangulationSearch.h): SearchForTriangulation of a new key frame against all its
neighbours in one device call.  tests/native_trisearch/test_trisearch_mock.cpp runs the class against a host model of the entry
points it calls (no device: set identity, the limit raise, concatenation order, epipoles, pair order; also under
AddressSanitizer / UBSan); test_trisearch_dropin.cpp runs it on the device against K calls of ORBmatcher::SearchForTriangulation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_trisearch")


def _run(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_trisearch/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and ("%s: OK" % name.replace("_asan", "")) in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_class_against_a_host_model_of_the_entry_points():
    _run("test_trisearch_mock")


def test_class_against_the_host_model_under_sanitizers():
    _run("test_trisearch_mock_asan")


@pytest.mark.gpu
def test_dropin_equals_one_matcher_call_per_neighbour():
    _run("test_trisearch_dropin")
