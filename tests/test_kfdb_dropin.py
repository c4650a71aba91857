"""The C++ drop-in KeyFrameDatabase (include/orbhip/KeyFrameDatabase.h) through tests/native_kfdb/test_kfdb_dropin, a program
that calls it like LoopClosing::DetectLoop and Tracking::Relocalization, against tests/kfdb_model.py: the candidates of every
query and the six query fields written back on every key frame, stale mRelocScore included."""
import os
import subprocess

import numpy as np
import pytest

from kfdb_model import KF, Model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "native_kfdb", "test_kfdb_dropin")


def _bow_text(w, v):
    return "%d %s" % (len(w), " ".join("%d %.17g" % (int(a), float(b)) for a, b in zip(w, v)))


def _f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_dropin_matches_the_reference(tmp_path):
    from orbhip import distributed as D
    if not os.path.exists(PROG):
        import __graft_entry__
        __graft_entry__.build()
    rng = np.random.default_rng(31)
    blob = D.make_synthetic_vocabulary(29, k=10, L=3)
    vocf = tmp_path / "voc.bin"
    vocf.write_bytes(blob)
    nwords = 1000
    base = []
    for _ in range(12):
        w = np.sort(rng.choice(nwords, 120, replace=False))
        v = rng.random(120)
        base.append((w, v / v.sum()))

    def variant(b, keep):
        w, v = b
        m = rng.random(len(w)) < keep
        m[0] = True
        v2 = v[m] * (1 + 0.3 * rng.random(m.sum()))
        return w[m], v2 / v2.sum()

    model = Model(nwords)
    kfs, live, lines, expect = {}, [], [], []
    qid = 10 ** 6
    for step in range(220):
        r = rng.random()
        if r < 0.4 or len(live) < 5:
            key = len(kfs) + 1
            b = variant(base[int(rng.integers(12))], 0.6)
            kf = KF(key, *b)
            kfs[key] = kf
            model.add(kf)
            live.append(kf)
            lines.append("add %d %s" % (key, _bow_text(*b)))
            n = min(10, len(live) - 1, int(rng.integers(0, 11)))
            others = [k for k in live if k is not kf]
            kf.covis = [others[i] for i in rng.choice(len(others), n, replace=False)] if n else []
            lines.append("covis %d %d %s" % (key, len(kf.covis), " ".join(str(c.key) for c in kf.covis)))
        elif r < 0.48:
            kf = live.pop(int(rng.integers(len(live))))
            model.erase(kf)
            lines.append("erase %d" % kf.key)
        elif r < 0.49:
            model.clear()
            live = []
            lines.append("clear")
        else:
            qid += 1
            q = variant(base[int(rng.integers(12))], 0.7)
            if r < 0.75:
                cand = model.detect_reloc(q, qid)
                lines.append("reloc %d %s" % (qid, _bow_text(*q)))
            else:
                conn = list(rng.choice(live, min(len(live), int(rng.integers(0, 8))), replace=False)) if live else []
                ms = float(rng.choice([0.0, 0.02]))
                cand = model.detect_loop(q, set(conn), ms, qid)
                lines.append("loop %d %.9g %s %d %s" % (qid, ms, _bow_text(*q), len(conn), " ".join(str(c.key) for c in conn)))
            expect.append(([k.key for k in cand],
                           [(k.key, k.mnLoopQuery, k.mnLoopWords, _f32_bits(k.mLoopScore), k.mnRelocQuery, k.mnRelocWords,
                             _f32_bits(k.mRelocScore)) for k in sorted(kfs.values(), key=lambda k: k.key)]))
    scen, out = tmp_path / "scenario.txt", tmp_path / "out.txt"
    scen.write_text("\n".join(lines) + "\n")
    subprocess.run([PROG, str(scen), str(out), str(vocf)], check=True, timeout=300)
    got, cur = [], None
    for line in out.read_text().splitlines():
        t = line.split()
        if t[0] == "cand":
            cur = ([int(x) for x in t[1:]], [])
            got.append(cur)
        else:
            cur[1].append((int(t[1]), int(t[2]), int(t[3]), int(t[4], 16), int(t[5]), int(t[6]), int(t[7], 16)))
    assert len(got) == len(expect)
    for i, (g, e) in enumerate(zip(got, expect)):
        assert g[0] == e[0], i
        assert g[1] == e[1], i
