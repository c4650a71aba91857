"""Known answers, computed by hand, for the model the device and the drop-in are compared with (tests/baproblem_model.py), and
for each of the model's named defects a scene that it changes: a kernel with that mistake cannot pass tests/test_baproblem_gpu.py,
which holds scenes of every one of these kinds."""
import pytest

import baproblem_model as BM
import localmap_collect_model as CM


def _scene():
    """Key frames put in descending key order (rows 0, 1, 2, ... go to 9, 7, 5, 4, 3).  Local: 5 and 9.
    p1: 3, 5, 7 | p2: 5 | p3 (bad): 5, 9 | p4: 4, 5, 9 | p5: 9 | p6: 3, 9.  Key frame 8 is erased again; 6 shares nothing."""
    w = CM.World()
    for p in range(1, 9):
        w.add_point(p, bad=p == 3)
    rows = {9: [3, 0, 4, 5, 6], 8: [1, 4], 7: [0, 1], 6: [7, 8], 5: [1, 2, 3, 4], 4: [4], 3: [6, 0, 1]}
    for kf in sorted(rows, reverse=True):
        w.put_kf(kf, rows[kf])
    row_of = {kf: r for r, kf in enumerate(sorted(rows, reverse=True))}
    w.erase_kf(8)
    return w, row_of


def test_the_scene_by_hand():
    w, _ = _scene()
    pts, off, edges, fixed = BM.ba_problem(w, [5, 9])
    assert pts == [1, 2, 4, 5, 6]
    assert fixed == [3, 7, 4]                              # 3 and 7 at p1, 4 at p4; 6 shares nothing, 8 is gone
    assert off == [0, 3, 4, 7, 8, 10]
    assert edges == [(2, 2), (0, 0), (3, 1),               # p1: key frames 3, 5, 7
                     (0, 1),                               # p2: 5 alone
                     (4, 0), (0, 3), (1, 2),               # p4: 4, 5, 9
                     (1, 3),                               # p5
                     (2, 0), (1, 4)]                       # p6: 3, 9
    # the other order of the local key frames: the points' order and every number change, the sets do not
    pts2, off2, edges2, fixed2 = BM.ba_problem(w, [9, 5])
    assert pts2 == [4, 5, 6, 1, 2] and fixed2 == [4, 3, 7] and len(edges2) == len(edges)
    # every key frame local (global BA): nothing is fixed
    assert BM.ba_problem(w, [3, 4, 5, 6, 7, 9])[3] == []
    assert BM.ba_problem(w, []) == ([], [0], [], [])
    assert BM.ba_problem(w, [6])[3] == []


def test_a_doubled_local_key_adds_nothing():
    w, _ = _scene()
    once, twice = BM.ba_problem(w, [5, 9]), BM.ba_problem(w, [5, 9, 5])
    assert twice[0] == once[0] and twice[1] == once[1]
    assert twice[3] == once[3]
    assert twice[2] == [(kf + 1 if kf >= 2 else kf, idx) for kf, idx in once[2]]   # fixed numbers start behind three keys


@pytest.mark.parametrize("defect", BM.DEFECTS)
def test_each_defect_changes_the_scene(defect):
    w, row_of = _scene()
    kfs = [5, 9, 5] if defect == "double_local" else [5, 9]
    ghosts = [(1, 4, 0)]                                   # as if key frame 4's entry 0 (point 4) named point 1's slot
    want = BM.ba_problem(w, kfs)
    got = BM.ba_problem(w, kfs, defect=defect, row_of=row_of, ghosts=ghosts)
    assert got != want
    changed = [name for name, a, b in zip(("points", "off", "edges", "fixed"), got, want) if a != b]
    expect = {"row_order": ["edges", "fixed"], "keep_bad": ["points", "off", "edges"], "stale": ["off", "edges", "fixed"],
              "local_as_fixed": ["edges", "fixed"], "fixed_by_key": ["edges", "fixed"], "double_local": ["edges"],
              "local_only": ["off", "edges", "fixed"]}
    assert changed == expect[defect]
