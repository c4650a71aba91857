"""The host code of the C ABI owns its GPU memory through one type, OrbBlock (csrc/orbhip_internal.h): a buffer is freed because
its owner goes away, not because someone remembered to add it to a free list.  No raw allocation or release may appear in code
anywhere else in csrc/ -- except orbhip_host_alloc / orbhip_host_free, public entry points that hand a block to the caller."""
import os
import re

from test_device_helpers import CSRC, _code, _sources

PAT = re.compile(r"\bhip(?:Host)?(?:Malloc|Free)(?:Async|Managed)?\b")
STRING = re.compile(r'"(?:\\.|[^"\\])*"')
# (file, the head of a definition in it that may call them; string literals are blanked before the match)
ALLOWED = [
    ("orbhip_internal.h", re.compile(r"\nstruct OrbBlock \{")),
    ("api_pipe.hip", re.compile(r"\bvoid \*orbhip_host_alloc\(")),
    ("api_pipe.hip", re.compile(r"\bvoid orbhip_host_free\(")),
]


def _strip(src):
    """code without comments or the text of string literals (error messages may name the call that failed)"""
    return STRING.sub('""', _code(src))


def _body(code, head):
    """[start, end) of the braced definition that `head` starts, or None"""
    m = head.search(code)
    if not m:
        return None
    i = code.index("{", m.start())
    depth = 0
    for j in range(i, len(code)):
        depth += {"{": 1, "}": -1}.get(code[j], 0)
        if depth == 0:
            return m.start(), j + 1
    raise AssertionError("unbalanced braces after " + head.pattern)


def _raw_calls(name, code):
    spans = [sp for sp in (_body(code, head) for f, head in ALLOWED if f == name) if sp]
    return [code.count("\n", 0, m.start()) + 1 for m in PAT.finditer(code)
            if not any(a <= m.start() < b for a, b in spans)]


def test_gpu_memory_is_allocated_and_freed_only_by_the_owning_type():
    found = []
    for path in _sources():
        name = os.path.basename(path)
        found += ["%s:%d" % (name, line) for line in _raw_calls(name, _strip(open(path).read()))]
    assert not found, "own the memory through OrbBlock (csrc/orbhip_internal.h) instead:\n" + "\n".join(found)


def test_the_allowed_definitions_exist_and_allocate():
    """The scan above is not vacuous: each exempted definition is there and holds a call the pattern matches."""
    for name, head in ALLOWED:
        code = _strip(open(os.path.join(CSRC, name)).read())
        span = _body(code, head)
        assert span and PAT.search(code[span[0]:span[1]]), (name, head.pattern)


def test_comments_and_strings_do_not_count_but_calls_elsewhere_do():
    src = '// hipFree(p)\n/* hipMalloc(&p, 4) */ fail(c, "hipHostMalloc (result block)");\n' \
          'struct OrbBlock { void f() { (void)hipFree(p); } };\nvoid g() { hipHostFree(q); }\n'
    assert _raw_calls("orbhip_internal.h", _strip(src)) == [4]
