#!/usr/bin/env python3
"""The public declarations of the drop-in headers include/orbhip/ORBextractor.h / ORBmatcher.h against those of the
reference's include/ORBextractor.h / ORBmatcher.h.

The reference's declarations are kept as digests only, in tests/golden/dropin_decls.json (SHA-256 of each declaration after
removing comments and white space, and of the same with `std::` removed): nothing of the reference's text is stored.
  diff_dropin_headers.py                                 compare against the stored digests
  diff_dropin_headers.py --reference DIR                 compare against a reference tree read at run time
  diff_dropin_headers.py --reference DIR --write-golden  (re)write the stored digests from that tree
A declaration counts as
  identical   same text after removing comments and white space,
  std-only    same after also removing `std::` (the reference headers rely on `using namespace std` leaking in),
  missing     in the reference class, not in the drop-in (exit code 1),
  extra       only in the drop-in (reported; additions such as SetDevice are allowed).
"""
import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_decls.json")
PAIRS = [("ORBextractor", "include/orbhip/ORBextractor.h", "include/ORBextractor.h"),
         ("ORBmatcher", "include/orbhip/ORBmatcher.h", "include/ORBmatcher.h")]


def class_body(text, name):
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bclass\s+%s\b[^;{]*\{" % name, text)
    if not m:
        return None
    i, depth = m.end(), 1
    while depth and i < len(text):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def declarations(body):
    """Statements of the class body by access section, inline function bodies dropped."""
    out, access, depth, cur = {"public": [], "protected": [], "private": []}, "private", 0, ""
    i = 0
    while i < len(body):
        ch = body[i]
        if depth == 0:
            m = re.match(r"\s*(public|protected|private)\s*:", body[i:])
            if m and not cur.strip():
                access = m.group(1)
                i += m.end()
                continue
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth == 0:          # end of an inline body: the declaration is what came before it
                out[access].append(cur)
                cur = ""
                i += 1
                while i < len(body) and body[i] in " \t\r\n;":
                    i += 1
                continue
        elif depth == 0:
            if ch == ";":
                out[access].append(cur)
                cur = ""
            else:
                cur += ch
        i += 1
    norm = lambda s: re.sub(r"\s+", "", s)
    return {k: [norm(d) for d in v if norm(d)] for k, v in out.items()}


def digest(decl):
    return hashlib.sha256(decl.encode()).hexdigest()


def nostd(decl):
    return decl.replace("std::", "")


def reference_digests(ref):
    """{class: {section: [[digest, digest without std::], ...]}} of the reference tree `ref`; None for a class not found."""
    out = {}
    for name, _, theirs in PAIRS:
        b = class_body(open(os.path.join(ref, theirs)).read(), name)
        out[name] = None if b is None else {sec: [[digest(d), digest(nostd(d))] for d in decls]
                                              for sec, decls in declarations(b).items() if sec != "private"}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", default=None, help="reference tree to read instead of the stored digests")
    ap.add_argument("--write-golden", action="store_true", help="write the digests of --reference to " + GOLDEN)
    args = ap.parse_args()
    if args.reference:
        ref = reference_digests(args.reference)
        if args.write_golden:
            with open(GOLDEN, "w") as fh:
                json.dump(ref, fh, indent=1, sort_keys=True)
                fh.write("\n")
            print("wrote " + GOLDEN)
            return 0
    else:
        ref = json.load(open(GOLDEN))
    rc = 0
    for name, mine, _ in PAIRS:
        a = class_body(open(os.path.join(ROOT, mine)).read(), name)
        if a is None or ref.get(name) is None:
            print("%s: class not found" % name)
            rc = 1
            continue
        A = declarations(a)
        for sec in ("public", "protected"):
            mine_set = {digest(d) for d in A[sec]}
            mine_nostd = {digest(nostd(d)) for d in A[sec]}
            B = ref[name][sec]
            ident = [d for d, _ in B if d in mine_set]
            stdonly = [d for d, n in B if d not in mine_set and n in mine_nostd]
            missing = [d for d, n in B if d not in mine_set and n not in mine_nostd]
            ref_nostd = {n for _, n in B}
            extra = [d for d in A[sec] if digest(nostd(d)) not in ref_nostd]
            print("%-13s %-9s reference %2d: identical %2d, std-only %2d, missing %2d; extra in the drop-in %2d"
                  % (name, sec, len(B), len(ident), len(stdonly), len(missing), len(extra)))
            for d in missing:
                print("    MISSING  sha256 " + d)
                if sec == "public":
                    rc = 1
            for d in extra:
                print("    extra    " + d)
    return rc


if __name__ == "__main__":
    sys.exit(main())
