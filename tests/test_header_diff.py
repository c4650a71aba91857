"""Public declarations of the drop-in classes against the reference's headers: tools/diff_dropin_headers.py compares the drop-in
headers with the digests of the reference's declarations stored in tests/golden/dropin_decls.json (no reference text is kept)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_public_declaration_of_the_reference_classes_has_a_dropin():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "diff_dropin_headers.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if " public " in l]
    assert len(lines) == 2 and all("missing  0" in l for l in lines), out.stdout
