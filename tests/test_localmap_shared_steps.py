"""The steps the LocalMapSearch drop-ins share have one definition each.  The room a call offers first and
the call made again are tested on their own (tests/native_shared_steps/test_room_retry.cpp: no mock returns ORBHIP_E_CAPACITY to
SearchLoopPoints, so that program is what covers the shared loop), plain and under AddressSanitizer / UBSan; a comment-stripped
scan of host/localmap/*.cc, in the manner of tests/test_shared_rules.py, keeps the definitions single."""
import glob
import os
import re
import subprocess

import pytest

from test_device_helpers import _code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_shared_steps")
LOCALMAP = os.path.join(ROOT, "vi-orb-slam-icra2018_amd", "host", "localmap")

# pattern -> the only .cc file it may appear in (None: in none; its one definition is in LocalMapDetail.h)
SHARED_STEPS = {
    "a lookup in mPointOf": (re.compile(r"mPointOf\.(find|count|end|erase)\("), "LocalMap.cc"),
    "a lookup in mKeyFrameOf": (re.compile(r"mKeyFrameOf\.(find|count|end|erase)\("), "LocalMapCollect.cc"),
    "a capacity retry": (re.compile(r"ORBHIP_E_CAPACITY"), "LocalMapBA.cc"),
    "the observation order": (re.compile(r"struct\s+ByMnId"), None),
    "a stopwatch": (re.compile(r"steady_clock"), None),
}


def _drop_ins():
    return sorted(glob.glob(os.path.join(LOCALMAP, "*.cc")))


@pytest.mark.parametrize("name", ["test_room_retry", "test_room_retry_asan"])
def test_room_and_retry_on_their_own(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_shared_steps/%s is not built (run __graft_entry__.build())" % name
    out = subprocess.run([p], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok" and not out.stderr.strip(), out.stdout + out.stderr


def test_shared_steps_are_written_only_in_their_homes():
    found = []
    for path in _drop_ins():
        code = _code(open(path).read())
        for name, (pat, home) in SHARED_STEPS.items():
            if os.path.basename(path) == home:
                continue
            for m in pat.finditer(code):
                found.append("%s:%d: %s (%s has it)" % (os.path.basename(path), code.count("\n", 0, m.start()) + 1, name,
                                                        home or "LocalMapDetail.h"))
    assert not found, "use the shared definition instead:\n" + "\n".join(found)


def test_the_step_patterns_match_their_homes():
    """The scan above is not vacuous: it reaches every file of the directory (twelve .cc files; the thirteenth file is
    LocalMapDetail.h, the home that is read here), and every pattern matches its home's own code."""
    names = [os.path.basename(p) for p in _drop_ins()]
    assert names == sorted("LocalMap%s.cc" % s for s in ("", "BA", "BowCand", "Collect", "Correct", "Covis", "Cull", "Fuse", "Loop",
                                                         "ProjTrack", "Refresh", "Sim3")), names
    assert sorted(f for f in os.listdir(LOCALMAP) if f.endswith((".cc", ".h"))) == sorted(names + ["LocalMapDetail.h"])
    for name, (pat, home) in SHARED_STEPS.items():
        assert pat.search(_code(open(os.path.join(LOCALMAP, home or "LocalMapDetail.h")).read())), name
    assert SHARED_STEPS["a lookup in mPointOf"][0].search("if (!mPointOf.count(key_of(p))) continue;") and \
        not SHARED_STEPS["a lookup in mPointOf"][0].search("room_for(mnLastLocal, mPointOf.size())")
