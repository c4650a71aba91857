"""The Fuse model (tests/fuse_model.py) on the CPU: the scenes of tests/fuse_scenes.py contain what tests/test_fuse_gpu.py relies
on -- every exit of the projection loop, enough fused candidates, both chi-square gates deciding both ways, the edge cases each
ending where it is meant to, and a point on which the two associations of u disagree across a bound."""
import numpy as np
import pytest

import fuse_model as FM
import fuse_scenes as S

f32 = np.float32


@pytest.fixture(scope="module")
def main_scene(oracle):
    return S.make(oracle)


def test_main_scene_reaches_every_exit_and_both_gates(oracle, main_scene):
    sc = main_scene
    st = S.model_store(sc)
    seen, fused = set(), 0
    for k, T in enumerate(sc["targets"]):
        stats = {}
        q, code, qd, na, bi, bd = FM.fuse(oracle, st, T, T["th"], sc["row"], sc["skip"][k], stats)
        seen |= set(int(c) for c in code)
        fused += int((bd <= FM.TH_LOW).sum())
        assert na == int((q["flags"] & FM.Q_ACTIVE).astype(bool).sum()) and na >= 100
        assert ((bi < 0) == (bd == 256)).all() and (bi[~(q["flags"] & 1).astype(bool)] == -1).all()
        assert stats["mono_pass"] >= 10 and stats["mono_out"] >= 10
        if T["u_right"] is not None:
            assert stats["stereo_pass"] >= 10 and stats["stereo_out"] >= 10
        else:
            assert stats["stereo_pass"] == 0 and stats["stereo_out"] == 0
        if k == 0:
            assert int((bd <= FM.TH_LOW).sum()) >= 50
    # every exit of the reference's loop; NONFINITE (a stated divergence) is the edge scene's
    assert seen == set(range(len(FM.EXITS))) - {FM.NONFINITE}
    assert fused >= 250
    # targets 0 and 3 share a set but not th: their windows differ
    a = FM.fuse_queries(st, sc["targets"][0]["cam"], sc["targets"][0]["th"], sc["row"])[0]
    b = FM.fuse_queries(st, sc["targets"][3]["cam"], sc["targets"][3]["th"], sc["row"])[0]
    assert np.array_equal(a["u"], b["u"]) and (a["radius"] != b["radius"]).any()
    assert len({len(T["kps"]) for T in sc["targets"]}) == 4


def test_edge_scene_cases_end_where_they_are_meant_to(oracle):
    sc = S.edge_scene()
    ix, T = sc["ix"], sc["targets"][0]
    st = S.model_store(sc)
    stats = {}
    q, code, qd, na, bi, bd = FM.fuse(oracle, st, T, T["th"], sc["row"], sc["skip"][0], stats)
    for case, want in S.EDGE_EXPECT.items():
        if want is None:
            assert code[ix[case]] != FM.ACTIVE, case
        else:
            assert code[ix[case]] == want, (case, FM.EXITS[code[ix[case]]])
    assert FM.NONFINITE in code and int((bd <= FM.TH_LOW).sum()) >= 10
    # the bounds: the minimum is inside, the maximum is outside
    b = S.EDGE_BOUNDS
    assert q["u"][ix["u_min"]] == b[0] and q["v"][ix["v_min"]] == b[2]
    assert q["u"][ix["u_max_below"]] == np.nextafter(b[1], f32(0)) and q["v"][ix["v_max_below"]] == np.nextafter(b[3], f32(0))
    # the level clamp at both ends, and the gate cases on the levels their sigma was made for
    assert q["max_level"][ix["level_low"]] == 0 and q["max_level"][ix["level_high"]] == S.LS.NLEVELS - 1
    for case, lv in S.GATE_LEVELS.items():
        assert q["max_level"][ix[case]] == lv, case
    # the gates: the product is the largest float not above the limit (kept) or the float after it (dropped)
    for lim, on, out in ((5.99, "gate_mono_on", "gate_mono_out"), (7.8, "gate_stereo_on", "gate_stereo_out")):
        lo, hi = S.gate_limits(lim)
        assert float(lo) <= lim < float(hi)
        assert f32(f32(4) * T["sig"][S.GATE_LEVELS[on]]) == lo and f32(f32(4) * T["sig"][S.GATE_LEVELS[out]]) == hi
        assert bi[ix[on]] == ix[on] and bi[ix[out]] == -1
        assert q["u"][ix[on]] - T["kps"]["x"][ix[on]] == 2 and q["v"][ix[on]] == T["kps"]["y"][ix[on]]
    assert T["u_right"][ix["gate_stereo_on"]] == q["proj_xr"][ix["gate_stereo_on"]] >= 0
    assert stats["mono_out"] == 1 and stats["stereo_out"] == 1 and stats["stereo_pass"] == 1
    # the viewing limit: PO . n is exactly half the distance, and one float less
    assert bi[ix["view_on"]] == ix["view_on"] and bi[ix["inside"]] == ix["inside"]
    # a skip byte, a bad flag, an empty entry and an erased point: nothing of theirs reaches the search
    for case in ("skipped", "bad", "key0", "stale"):
        assert not q[ix[case]].tobytes().strip(b"\0") and bi[ix[case]] == -1


def test_association_of_u_decides_a_bound(oracle):
    sc, ua, ub = S.assoc_scene()
    T = sc["targets"][0]
    st = S.model_store(sc)
    assert ua != ub and T["cam"]["bounds"][1] == max(ua, ub)
    fuse_way = FM.fuse_queries(st, T["cam"], T["th"], sc["row"])
    other_way = FM.fuse_queries(st, T["cam"], T["th"], sc["row"], other_association=True)
    inside = {bool(fuse_way[1][0] == FM.ACTIVE), bool(other_way[1][0] == FM.ACTIVE)}
    assert inside == {True, False}                      # different sides of mnMaxX
    assert {int(fuse_way[1][0]), int(other_way[1][0])} == {FM.ACTIVE, FM.RIGHT}
    assert (fuse_way[1][0] == FM.ACTIVE) == (ua < ub)   # Fuse's own value is the one the device must reproduce


def test_collect_model_keeps_first_occurrences_in_order(oracle, main_scene):
    sc = main_scene
    st = S.model_store(sc)
    rows = [sc["row"][:200], sc["row"][100:350][::-1], sc["row"][300:]]
    got = FM.collect(st, rows)
    assert len(got) == len(set(got.tolist())) and 0 not in got
    live = [int(k) for r in rows for k in r if int(k) and int(k) in st.pts and not st.pts[int(k)][5] & 2]
    assert set(got.tolist()) == set(live) and got[0] == live[0]
    assert 250 < len(got) < len(live)
