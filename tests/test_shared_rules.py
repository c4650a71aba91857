"""The rules of the projection arithmetic, of the rotation check and of the chi-square gate that docs/parity.md declares bit-exact
live in one device header each.  The comment-stripped scan of tests/test_device_helpers.py over the kernel
files and the headers of csrc/: none of them may appear in code anywhere else.  api_*.hip is host code and is not scanned
(api_match.hip's orb_three_maxima stays)."""
import glob
import os
import re

from test_device_helpers import CSRC, _code

# pattern -> its home
SHARED_RULES = {
    "cv::norm's double square root": (re.compile(r"__dsqrt_rn"), "project_dev.h"),
    "PredictScale's table loop": (re.compile(r"level_ratio\s*\["), "project_dev.h"),
    "ComputeThreeMaxima's ladder": (re.compile(r"max3\s*=\s*max2\s*;\s*max2\s*=\s*max1"), "bow_rot_dev.h"),
    "chi-square limit 5.99": (re.compile(r"(?<![\w.])5\.99(?![\w.])"), "localmap_dev.h"),
    "chi-square limit 7.8": (re.compile(r"(?<![\w.])7\.8(?![\w.])"), "localmap_dev.h"),
}


def _device_sources():
    return sorted(glob.glob(os.path.join(CSRC, "k_*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_shared_rules_are_defined_only_in_their_headers():
    found = []
    for path in _device_sources():
        code = _code(open(path).read())
        for name, (pat, home) in SHARED_RULES.items():
            if os.path.basename(path) == home:
                continue
            for m in pat.finditer(code):
                found.append("%s:%d: %s (csrc/%s has it)" % (os.path.basename(path), code.count("\n", 0, m.start()) + 1, name, home))
    assert not found, "use the shared definition instead:\n" + "\n".join(found)


def test_the_rule_patterns_match_their_headers():
    """The scan above is not vacuous: every pattern matches its home's own code, and the scan reaches the kernel files."""
    names = [os.path.basename(p) for p in _device_sources()]
    assert {"k_guided.hip", "k_fuse.hip", "k_localmap.hip", "refresh_dev.h", "project_dev.h", "bow_rot_dev.h", "localmap_dev.h"} <= set(names)
    for name, (pat, home) in SHARED_RULES.items():
        assert pat.search(_code(open(os.path.join(CSRC, home)).read())), name
    assert not SHARED_RULES["chi-square limit 5.99"][0].search("#define IS_TH_H 5.991f") and \
        SHARED_RULES["chi-square limit 5.99"][0].search("double lim = 5.99;")
