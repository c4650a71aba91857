"""tests/kfdb_model.py (the restatement of src/KeyFrameDatabase.cc that the device database is checked against) on
hand-built cases, and the drop-in's KeyFrameDatabase.cc compiled for syntax against both cv front ends.  CPU only."""
import os
import subprocess

import numpy as np

from kfdb_model import KF, Model, l1_score, min_common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bow(d):
    w = sorted(d)
    return (w, [d[k] for k in w])


def test_l1_known_answers():
    a = bow({1: 0.25, 4: 0.25, 9: 0.5})
    assert l1_score(a, a) == 1.0
    assert l1_score(a, bow({2: 0.5, 3: 0.5})) == 0.0
    # common words 4 and 9: |.25-.5|-.25-.5 + |.5-.25|-.5-.25 = -.5 -.5 -> score 0.5
    assert l1_score(a, bow({4: 0.5, 9: 0.25, 11: 0.25})) == 0.5


def test_min_common_is_a_float_product_truncated():
    assert min_common(5) == 4            # 5 * 0.8f = 4.0000...  -> 4, and the test is strict: 4 shared words are too few
    assert min_common(1) == 0 and min_common(10) == 8 and min_common(3) == 2
    m = Model(20)
    full = bow({i: 0.2 for i in range(5)})
    a, b = KF(1, *full), KF(2, *bow({i: 0.25 for i in range(4)}))
    m.add(a)
    m.add(b)
    out, minc = m.score(0, full)
    assert minc == 4 and [(k, c) for k, c, _ in out] == [(1, 5), (2, 4)]
    assert out[1][2] == 0                # not scored


def test_first_occurrence_order():
    m = Model(10)
    k1, k2, k3 = KF(1, *bow({5: 1.0})), KF(2, *bow({2: 0.5, 5: 0.5})), KF(3, *bow({2: 1.0}))
    for k in (k1, k2, k3):
        m.add(k)
    out, _ = m.score(0, bow({2: 0.5, 5: 0.5}))
    assert [k for k, _, _ in out] == [2, 3, 1]        # word 2's list first (add order), then word 5's newcomers


def test_dedupe_through_the_best_covisible():
    m = Model(10)
    q = bow({1: 0.5, 2: 0.5})
    a, b, c = KF(1, *q), KF(2, *bow({1: 0.45, 2: 0.55})), KF(3, *bow({1: 0.6, 2: 0.4}))
    for k in (a, b, c):
        m.add(k)
    c.covis = [a]
    b.covis = [a]
    # b and c are retained, both through their best covisible key frame a (score 1.0): one candidate
    assert [k.key for k in m.detect_reloc(q)] == [1]


def test_loop_excludes_connected_key_frames():
    m = Model(10)
    q = bow({1: 0.5, 2: 0.5})
    a, b = KF(1, *q), KF(2, *bow({1: 0.4, 2: 0.6}))
    m.add(a)
    m.add(b)
    assert [k.key for k in m.detect_loop(q, {a}, 0.0)] == [2]
    assert a.mnLoopWords == 1 and a.mnLoopQuery == 0            # reset on every visit, never stamped
    assert [k.key for k in m.detect_loop(q, {a, b}, 0.0)] == []


def test_stale_reloc_score_changes_the_answer():
    def run(stale_first):
        m = Model(30)
        x = KF(1, *bow({1: 0.5, 2: 0.5}))
        y = KF(2, *bow({10: 0.5, 11: 0.5, 1: 0.0 + 1e-9}))   # shares one word with the second query
        z = KF(3, *bow({1: 0.5, 3: 0.5}))
        for k in (x, y, z):
            m.add(k)
        x.covis = [y]
        z.covis = [y]
        if stale_first:
            m.detect_reloc(bow({10: 0.5, 11: 0.5}))          # scores y highly: its mRelocScore stays
        return [k.key for k in m.detect_reloc(bow({1: 0.5, 3: 0.3, 4: 0.2}))], y.mRelocScore

    fresh, s0 = run(False)
    stale, s1 = run(True)
    assert s0 == 0 and s1 > 0.9
    # y shares one word with the second query but is not scored there: its stale score becomes z's pBestKF
    assert fresh == [3] and stale == [2]


def test_dropin_body_compiles():
    src = os.path.join(ROOT, "vi-orb-slam-icra2018_amd", "host", "kfdb", "KeyFrameDatabase.cc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "orbhip")]
    stub = "-I" + os.path.join(ROOT, "tests", "native", "opencv_stub")
    for extra in ([], ["-DORBHIP_USE_OPENCV", stub]):
        subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Werror"] + inc + extra + [src], check=True)


def test_header_declares_the_reference_surface():
    h = open(os.path.join(ROOT, "include", "orbhip", "KeyFrameDatabase.h")).read()
    for decl in ("KeyFrameDatabase(const ORBVocabulary &voc);", "void add(KeyFrame *pKF);", "void erase(KeyFrame *pKF);",
                 "void clear();", "std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);",
                 "std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);"):
        assert decl in h, decl
    assert "class KeyFrameDatabase" in h and "namespace ORB_SLAM2" in h
