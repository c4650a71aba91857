"""The model of LoopClosing's projection searches (tests/loopfuse_model.py) on the CPU: the scenes of tests/loopfuse_scenes.py contain
what tests/test_loopfuse_gpu.py relies on -- every exit of both loops, the edge cases each ending where it is meant to, a best
feature that the chi-square gate would have refused, a point held by one target and free in another, a stale row entry whose slot
went to a point of the list, and every turn of the sequential claim."""
import numpy as np
import pytest

import fuse_model as FM
import loopfuse_model as LM
import loopfuse_scenes as S

f32 = np.float32


@pytest.fixture(scope="module")
def main_scene():
    return S.make()


@pytest.fixture(scope="module")
def main_result(oracle, main_scene):
    sc = main_scene
    return LM.fuse_sim3(oracle, S.model_store(sc), sc["targets"], S.target_rows(sc), sc["loop"])


def test_scene_shapes(main_scene):
    sc = main_scene
    assert sorted(len(k) for k, _ in sc["sets"].values()) == [1, 17, 33, 50]
    assert sc["targets"][0]["key"] == sc["targets"][3]["key"] and sc["targets"][0]["th"] != sc["targets"][3]["th"]
    assert not np.array_equal(sc["targets"][0]["cam"]["Rcw"], sc["targets"][3]["cam"]["Rcw"])      # one set under two similarities
    assert len(sc["loop"]) >= max(S.SIZES) and S.ROWS[2] == 0
    nz = sc["loop"][sc["loop"] != 0]
    assert len(set(nz.tolist())) == len(nz)                                                          # no key twice
    for T in sc["targets"]:
        assert all(0 <= T["kps"][a].min() and T["kps"][a].max() < 128 for a in ("x", "y"))
    assert set(float(s) for s in S.SCALES) == {0.5, float(f32(1.37)), 2.0}


def test_decomposition_rounds_and_agrees_with_the_definition():
    rng = np.random.default_rng(5)
    R, t, _ = S.LS.pose(rng, 0.3, 0.5)
    for s in (0.5, 1.37, 2.0):
        Scw = LM.sim3(s, R, t)
        Rcw, tcw, Ow, scw = LM.decompose_sim3(Scw)
        assert abs(float(scw) - s) < 1e-6 and np.allclose(Rcw, R, atol=1e-6) and np.allclose(tcw, t, atol=1e-6)
        assert np.allclose(Ow, -(R.astype(np.float64).T @ t.astype(np.float64)), atol=1e-6)


def test_main_scene_reaches_every_exit(oracle, main_scene, main_result):
    sc = main_scene
    seen = set()
    for k, (q, code, qd, na, bi, bd) in enumerate(main_result):
        seen |= set(int(c) for c in code)
        assert na == int((q["flags"] & LM.Q_ACTIVE).astype(bool).sum())
        assert ((bi < 0) == (bd == 256)).all() and (bi[~(q["flags"] & 1).astype(bool)] == -1).all()
        assert not q["proj_xr"].any()
        if S.ROWS[k]:
            assert (code == LM.SKIPPED).sum() >= 5
        else:
            assert not (code == LM.SKIPPED).any()
    assert seen == set(range(len(FM.EXITS))) - {FM.NONFINITE}
    assert sum(int((r[5] <= LM.TH_LOW).sum()) for r in main_result) >= 100 and all(r[3] >= 50 for r in main_result[:2])


def test_gate_off_finds_another_feature_than_gate_on(oracle, main_scene, main_result):
    sc = main_scene
    differ = 0
    for T, (q, code, qd, na, bi, bd) in zip(sc["targets"], main_result):
        gi, gd = FM.window_best_gated(oracle, T["kps"], T["desc"], T["gp"], q, qd, None, T["sig"])
        differ += int(((gi != bi) & (bi >= 0) & (gi >= 0)).sum())
        assert (bd <= gd).all()
    assert differ >= 1


def test_held_in_one_target_free_in_another_and_stale_entries(oracle, main_scene, main_result):
    sc = main_scene
    codes = np.stack([r[1] for r in main_result])
    assert (((codes == LM.SKIPPED).any(axis=0)) & ((codes == LM.ACTIVE).any(axis=0))).sum() >= 5
    # the first target's row holds entries whose points left the map; the new points in their slots are in the list and take part
    st = S.model_store(sc)
    row0 = sc["rows"][S.ROWS[0]]
    stale_in_row = [int(k) for k in sc["keys"][sc["stale"][:4]] if int(k) in set(row0.tolist())]
    assert len(stale_in_row) == 4 and all(k not in st.pts for k in stale_in_row)
    pos = {int(k): i for i, k in enumerate(sc["loop"])}
    fresh_at = [pos[int(k)] for k in sc["fresh_keys"][:4]]
    assert (codes[0][fresh_at] != LM.SKIPPED).all() and (codes[0][fresh_at] == LM.ACTIVE).any()
    assert all(codes[0][pos[k]] == LM.UNKNOWN for k in stale_in_row)


def test_edge_scene_cases_end_where_they_are_meant_to(oracle):
    sc = S.edge_scene()
    ix = sc["ix"]
    (q, code, qd, na, bi, bd), = LM.fuse_sim3(oracle, S.model_store(sc), sc["targets"], S.target_rows(sc), sc["loop"])
    for case, want in S.EDGE_EXPECT.items():
        if want is None:
            assert code[ix[case]] != LM.ACTIVE, case
        else:
            assert code[ix[case]] == want, (case, FM.EXITS[code[ix[case]]])
    b = S.EDGE_BOUNDS
    assert q["u"][ix["u_min"]] == b[0] and q["v"][ix["v_min"]] == b[2]
    assert q["u"][ix["u_max_below"]] == np.nextafter(b[1], f32(0)) and q["v"][ix["v_max_below"]] == np.nextafter(b[3], f32(0))
    assert q["max_level"][ix["level_low"]] == 0 and q["max_level"][ix["level_high"]] == S.LS.NLEVELS - 1
    assert FM.NONFINITE in code and int((bd <= LM.TH_LOW).sum()) >= 10
    # the same list through the other search: the held point is free there, a matched one is not
    T = sc["targets"][0]
    matched = np.zeros(len(T["kps"]), np.uint64)
    matched[0] = sc["keys"][ix["inside"]]
    q2, code2, _ = LM.queries(S.model_store(sc), T["cam"], T["th"], sc["loop"], {int(matched[0])})
    assert code2[ix["inside"]] == LM.SKIPPED and code2[ix["held"]] == LM.ACTIVE
    assert all(code2[ix[c]] == code[ix[c]] for c in S.EDGE_CASES if c not in ("inside", "held"))


def test_claim_scene_takes_every_turn(oracle):
    sc = S.claim_scene()
    ix, T = sc["ix"], sc["targets"][0]
    trace = []
    keys, q, code, qd, na, nm, match = LM.search_loop_points(oracle, S.model_store(sc), T, list(sc["loop_rows"].values()), sc["matched"],
                                                           trace=trace)
    assert np.array_equal(keys, sc["keys"])                                      # the union keeps the first occurrence
    tr = {i: (got, best, free) for i, got, best, free in trace}
    assert tr[ix["first"]][0] == 0 and tr[ix["second"]] == (1, 15, 0)            # the same best feature: the later takes its next best
    assert tr[ix["third"]][0] == -1 and tr[ix["third"]][2] == 0                  # and the one after that has none
    assert tr[ix["closed_best"]] == (3, 20, 2)                                   # feature 2 is closed and would have been the best
    assert code[ix["matched"]] == LM.SKIPPED and ix["matched"] not in tr         # a point among vpMatched
    assert np.array_equal(qd[ix["tie_a"]], qd[ix["tie_b"]]) and tr[ix["tie_a"]][0] == 4 and tr[ix["tie_b"]][0] == -1
    assert nm == 4 and match.tolist() == [ix["first"], ix["second"], -1, ix["closed_best"], ix["tie_a"]]


def test_main_scene_claims(oracle, main_scene):
    sc = main_scene
    trace = []
    keys, q, code, qd, na, nm, match = LM.search_loop_points(oracle, S.model_store(sc), sc["targets"][0], list(sc["loop_rows"].values()),
                                                           sc["matched"], trace=trace)
    assert len(keys) >= 200 and na >= 50 and nm >= 10 and nm == int((match >= 0).sum())
    assert (code == LM.SKIPPED).sum() >= 3
    assert sum(1 for i, got, best, free in trace if got >= 0 and free >= 0 and got != free) >= 3     # a next best was taken
    assert sum(1 for i, got, best, free in trace if got < 0 and free >= 0) >= 3
    assert {LM.ACTIVE, FM.BEHIND, FM.LEFT, FM.RIGHT, FM.TOP, FM.BOTTOM, FM.NEAR, FM.FAR, FM.VIEW, LM.SKIPPED} <= set(int(c) for c in code)
