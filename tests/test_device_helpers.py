"""The kernels share one definition of each low-level wave primitive (csrc/wave_ops.h).  Two of them are easy to copy back into
a kernel file and hard to get right there: the LDS-DMA asm, whose M0 save / set / restore and hazard nop must stay in one
statement, and the DPP row_shr steps of the prefix sums.  Neither may appear in code anywhere else in csrc/."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vi-orb-slam-icra2018_amd", "csrc")
HOME = "wave_ops.h"

PATTERNS = {
    "LDS-DMA asm": re.compile(r"\\tglobal_load_lds_dword"),
    "DPP row_shr step": re.compile(r"__builtin_amdgcn_update_dpp\(\s*[^,()]+,\s*[^,()]+,\s*0x11[1248]\s*,"),
}


def _code(src):
    """src with its comments removed (string literals kept: the asm text lives in one)."""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if c == '"':
            j = i + 1
            while j < n and src[j] != '"':
                j += 2 if src[j] == "\\" else 1
            out.append(src[i:j + 1])
            i = j + 1
        elif src.startswith("//", i):
            j = src.find("\n", i)
            i = n if j < 0 else j
        elif src.startswith("/*", i):
            j = src.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("\n" * src.count("\n", i, j))   # keep the line numbers
            i = j
        else:
            out.append(c)
            i += 1
    return "".join(out)


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def test_wave_primitives_are_defined_only_in_the_shared_header():
    found = []
    for path in _sources():
        if os.path.basename(path) == HOME:
            continue
        code = _code(open(path).read())
        for name, pat in PATTERNS.items():
            for m in pat.finditer(code):
                found.append("%s:%d: %s" % (os.path.basename(path), code.count("\n", 0, m.start()) + 1, name))
    assert not found, "use the definitions in csrc/%s instead:\n%s" % (HOME, "\n".join(found))


def test_the_patterns_match_the_shared_definitions():
    """The scan above is not vacuous: both patterns match the header's own code."""
    code = _code(open(os.path.join(CSRC, HOME)).read())
    for name, pat in PATTERNS.items():
        assert pat.search(code), name


def test_comments_do_not_count():
    src = '// global_load_lds_dwordx4 \\tglobal_load_lds_dword __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true)\n' \
          '/* __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true) */ int m = 0x11111111;\n'
    code = _code(src)
    assert not any(p.search(code) for p in PATTERNS.values()), code
