"""The model of SearchByBoW against candidate key frames (tests/bowcand_model.py) against the two other host implementations of
the pair search -- the C oracle (oracle/orb_oracle_py.search_by_bow, validity as bytes, strict = mode) and tests/pymodels.py --, and
the scenes of tests/bowcand_scenes.py against their names.  No GPU."""
import numpy as np
import pytest

import bowcand_model as M
import bowcand_scenes as S
import pymodels

f32 = np.float32


def _pairs(mode, fixed, cands):
    """(side 1, side 2) of every candidate, the frame of mode 0 given all-valid points"""
    if mode == 0:
        frame = dict(fixed, points=[M.Point(False, (0, 0, 0))] * len(fixed["desc"]))
        return [(c, frame) for c in cands]
    return [(fixed, c) for c in cands]


def _against_others(mode, fixed, cands, p):
    import orb_oracle_py as oracle
    th, ratio, ori = p.get("th", 50), p.get("nnratio", 0.75), p.get("check_ori", True)
    want = M.candidates(mode, fixed, cands, th, ratio, ori)
    for k, (s1, s2) in enumerate(_pairs(mode, fixed, cands)):
        v1, v2 = M.valid_bytes(s1), (None if mode == 0 else M.valid_bytes(s2))
        n, m12, m21 = oracle.search_by_bow(s1["desc"], v1, s1["angle"], M.csr(s1["fv"]), s2["desc"], v2, s2["angle"], M.csr(s2["fv"]), th,
                                           mode, ratio, ori)
        pn, p12, p21 = pymodels.search_by_bow(s1["desc"], v1, s1["angle"], s1["fv"], s2["desc"], v2, s2["angle"], s2["fv"], th, mode == 1,
                                              ratio, ori)
        row = m21 if mode == 0 else m12
        assert want["matches"][k] == [int(x) for x in row] == (p21 if mode == 0 else p12)
        assert want["nmatches"][k] == n == pn == sum(1 for x in row if x >= 0)


SCENES = {
    "sizes_1": lambda m: S.node_sizes(m, 1), "sizes_64": lambda m: S.node_sizes(m, 64), "sizes_65": lambda m: S.node_sizes(m, 65),
    "sizes_129": lambda m: S.node_sizes(m, 129), "side1_65": lambda m: S.node_sizes(m, 5, 65), "batch_5": lambda m: S.batch(m, 5),
    "twice": S.twice, "disjoint": S.disjoint, "threshold": S.threshold, "ratio_equal": S.ratio_equal,
    "ratio_next": lambda m: S.ratio_equal(m, 5), "tie": S.tie, "claimed": S.claimed, "rot_two_bins": S.rot_two_bins,
    "rot_second_below_tenth": S.rot_second_below_tenth, "rot_bin_30": S.rot_bin_30, "all_invalid": S.all_invalid,
}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_model_agrees_with_oracle_and_pymodels(name, mode):
    fixed, cands, p = SCENES[name](mode)
    _against_others(mode, fixed, cands, p)
    _against_others(mode, fixed, cands, dict(p, check_ori=False))


def _one(mode, scene, **over):
    fixed, cands, p = scene
    p = dict(p, **over)
    r = M.candidates(mode, fixed, cands, p.get("th", 50), p.get("nnratio", 0.75), p.get("check_ori", True))
    s1, s2 = _pairs(mode, fixed, cands)[0]
    return r["matches"][0], r["nmatches"][0], s1, s2


def _dists(s1, s2, node=7):
    return [[M.distance(s1["desc"][a], s2["desc"][b]) for b in s2["fv"][node]] for a in s1["fv"][node]]


@pytest.mark.parametrize("mode", [0, 1])
def test_scenes_are_what_their_names_say(mode):
    # threshold: the best distance is exactly th and the ratio passes; <= matches, < does not
    row, nm, s1, s2 = _one(mode, S.threshold(mode))
    d = sorted(_dists(s1, s2)[0])
    assert d[0] == 8 and f32(d[0]) < f32(0.75) * f32(d[1])
    assert nm == (1 if mode == 0 else 0)
    # ratio at equality: 3 against 0.75f * 4 exactly; one more on the second best matches
    row, nm, s1, s2 = _one(mode, S.ratio_equal(mode))
    d = sorted(_dists(s1, s2)[0])
    assert f32(d[0]) == f32(0.75) * f32(d[1]) and nm == 0
    assert _one(mode, S.ratio_equal(mode, 5))[1] == 1
    # tie: two candidates at the best distance; the winner is the lower list position, which is the HIGHER feature index
    row, nm, s1, s2 = _one(mode, S.tie(mode))
    d = _dists(s1, s2)[0]
    assert sorted(d)[0] == sorted(d)[1] and d.index(min(d)) == 1
    lst = s2["fv"][7]
    winner, other = lst[1], lst[2]
    assert winner > other and nm == 1
    i1 = s1["fv"][7][0]
    assert (row[winner] == i1) if mode == 0 else (row[i1] == winner)
    # claimed: both side-1 features are nearest to X; the second one ends on Y
    row, nm, s1, s2 = _one(mode, S.claimed(mode), check_ori=False)
    d = _dists(s1, s2)
    y, x = s2["fv"][7]
    a, b = s1["fv"][7]
    assert d[0].index(min(d[0])) == 1 and d[1].index(min(d[1])) == 1 and nm == 2
    assert ((row[x], row[y]) == (a, b)) if mode == 0 else ((row[a], row[b]) == (x, y))
    # rotation
    for scene, before, after in ((S.rot_two_bins, 5, 5), (S.rot_second_below_tenth, 12, 11), (S.rot_bin_30, 11, 10)):
        assert _one(mode, scene(mode), check_ori=False)[1] == before and _one(mode, scene(mode))[1] == after
    fixed, cands, _ = S.rot_bin_30(mode)
    s1, s2 = _pairs(mode, fixed, cands)[0]
    assert [M._bin(a, 0.0) for a in (900.0, 180.0, 270.0, 95.0)] == [0, 6, 9, 3] and f32(900.0) in s1["angle"]
    sizes = [0] * 30
    for a in s1["angle"]:
        sizes[M._bin(a, 0.0)] += 1
    assert sorted(i for i, s in enumerate(sizes) if s) == [0, 3, 6, 9] and M.three_maxima(sizes) == (6, 9, 0)
    fixed, cands, _ = S.rot_two_bins(mode)
    assert len({M._bin(a, 0.0) for a in _pairs(mode, fixed, cands)[0][0]["angle"]}) == 2   # fewer than three non-empty bins
    # all invalid: nothing matches
    assert _one(mode, S.all_invalid(mode))[1] == 0
    # disjoint: the middle candidate shares no node
    fixed, cands, _ = S.disjoint(mode)
    assert not set(fixed["fv"]) & set(cands[1]["fv"]) and set(fixed["fv"]) & set(cands[0]["fv"])
    # batch: the pairs of a candidate straddle a block of four waves
    fixed, cands, _ = S.batch(mode, 9)
    counts = [len(set(fixed["fv"]) & set(c["fv"])) for c in cands]
    assert counts == [3, 5, 2, 7, 1, 6, 3, 5, 9] and any(sum(counts[:k]) % 4 for k in range(1, 9))


def test_node_size_scenes_have_the_sizes():
    for mode in (0, 1):
        for n2 in (0, 1, 64, 65, 128, 129, 4097):
            fixed, cands, _ = S.node_sizes(mode, n2)
            s1, s2 = _pairs(mode, fixed, cands)[0]
            assert len(s2["fv"][4]) == n2 and len(s1["fv"][4]) == 3
            # the node under test matches, its last side-2 list entry included, and a claimed feature is wanted again
            assert S.node4_matches(mode, (fixed, cands, {})) >= min(n2, 2)
        fixed, cands, _ = S.node_sizes(mode, 5, 65)
        assert len(_pairs(mode, fixed, cands)[0][0]["fv"][4]) == 65


def test_gather_model_is_the_pnpsolver_walk():
    frame, cands, _ = S.gather_scene()
    sigma2 = S.SIGMA2
    r = M.candidates(0, frame, cands, gather=(6, sigma2, 5.991))
    assert r["nmatches"] == [6, 5, 6] and r["off"] == [0, 6, 6, 12]
    assert r["kp_idx"] == list(range(6)) * 2                      # the frame's features in ascending index
    assert {int(frame["octave"][i]) for i in r["kp_idx"]} == {0, S.NLEVELS - 1}
    for t, (i, j) in enumerate(zip(r["kp_idx"], r["kf_idx"])):
        assert r["P2D"][t] == (frame["x"][i], frame["y"][i]) and r["P3Dw"][t] == cands[0]["points"][j].pos
        assert r["max_err"][t] == f32(sigma2[frame["octave"][i]] * f32(5.991))
    assert M.candidates(0, frame, cands, gather=(7, sigma2, 5.991))["off"] == [0, 0, 0, 0]
    assert M.candidates(0, frame, cands, gather=(5, sigma2, 5.991))["off"] == [0, 6, 11, 17]
