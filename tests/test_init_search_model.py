"""CPU checks of the SearchForInitialization model (tests/init_search_model.py) and scenes (tests/init_search_scenes.py): the model
equals the oracle on every scene, every named defect of the model changes the result of at least one scene (so the scenes can see
that bug), the trace confirms what each scene claims to contain, and the LDS layout choice of k_init_assign is restated and
checked at the caps the device tests allocate."""
import numpy as np
import pytest

import init_search_model as M
import init_search_scenes as S

f32 = np.float32


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


@pytest.fixture(scope="module")
def results():
    """The model's result of every scene, computed once."""
    return {s["name"]: M.run(s) for s in S.all_scenes()}


def test_float_facts_the_scenes_rest_on():
    r = f32(0.8)
    for best, best2 in ((8, 10), (4, 5), (40, 50)):
        assert f32(best2) * r == f32(best)                         # the float product is exactly bestDist: '<' fails
        assert float(best) < float(f32(best2)) * float(r)          # the double product lies above it
    assert f32(7) < f32(10) * r
    assert f32(0.1) * f32(10) == f32(1) and float(f32(0.1)) * 10.0 > 1.0
    assert f32(0.1) * f32(11) > f32(1)
    assert f32(0.1) * f32(20) == f32(2) and float(f32(0.1)) * 20.0 > 2.0
    factor = f32(1) / f32(30)
    assert f32(15) * factor == f32(0.5) and f32(135) * factor == f32(4.5)
    below = f32(14.999999)
    assert below < f32(15) and below * factor == f32(0.5) and float(below) * float(factor) < 0.5
    assert M.rotation_bin(15, 0) == 1 and M.rotation_bin(15, 0, "bin_rint") == 0
    assert M.rotation_bin(135, 0) == 5 and M.rotation_bin(135, 0, "bin_rint") == 4
    assert M.rotation_bin(below, 0) == 1 and M.rotation_bin(below, 0, "bin_double") == 0
    assert M.rotation_bin(10, 350) == 1 and M.rotation_bin(10, 350, "no_wrap") == -11
    assert max(M.rotation_bin(a, 0) for a in (359.99997, 345.0, 344.99997)) == 12     # bin 30 cannot occur: factor is 1 / 30


def test_model_equals_oracle_on_every_scene(oracle, results):
    n = 0
    for s in S.all_scenes():
        want = results[s["name"]]
        got = oracle.search_for_initialization(s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], s["prev"], s["window"], s["nnratio"],
                                               s["check_ori"])
        assert _same(got, want), s["name"]
        # the initialiser's second call, with the vbPrevMatched of the first
        again = M.search(s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], want[2], s["window"], s["nnratio"], s["check_ori"])
        got = oracle.search_for_initialization(s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], want[2], s["window"], s["nnratio"],
                                               s["check_ori"])
        assert _same(got, again), s["name"]
        assert want[0] == (want[1] >= 0).sum()
        n += want[0]
    assert n > 2000


def test_every_defect_is_separated_by_a_named_scene(results):
    """Prints, per defect, the scenes whose result the defective model changes; a defect that no scene separates fails by name."""
    unseparated = []
    for defect in M.DEFECTS:
        hits = [s["name"] for s in S.all_scenes() if not _same(M.run(s, defect), results[s["name"]])]
        print("defect %-17s separated by %d scenes: %s" % (defect, len(hits), ", ".join(hits[:4])))
        if not hits:
            unseparated.append(defect)
    assert not unseparated, "no scene separates: " + ", ".join(unseparated)


def test_comparison_scene_decisions(results):
    """The rows of 'compare_0p8' in the order of comparison_scenes(): what decided each."""
    s = S.by_name("compare_0p8")
    n, m12, _, tr = results[s["name"]]
    t = tr[s["ix"]]
    want = [("accept", 50, M.INT_MAX), ("th_low", 51, M.INT_MAX), ("ratio", 8, 10), ("ratio", 4, 5), ("ratio", 40, 50),
            ("accept", 7, 10), ("accept", 20, M.INT_MAX), ("ratio", 8, 10), ("ratio", 40, 50), ("ratio", 12, 12), ("ratio", 12, 12),
            ("ratio", 10, 12), ("ratio", 8, 10),
            ("accept", 10, 26), ("accept", 20, M.INT_MAX), ("accept", 6, M.INT_MAX)]
    for row, (decided, best, best2) in zip(t, want):
        assert (row["decided"], row["best"], row["best2"]) == (decided, best, best2)
    a, b, c = s["ix"][13:16]
    assert tr["displaced"][c] == a and m12[a] == -1 and m12[b] >= 0 and m12[c] == tr["best_idx"][a]      # displaced, not re-matched
    assert tr["skip_eq"][b] == 1 and tr["owned_gt"][c] == 1 and tr["skip_lt"][c] == 1
    o1, o3, o0 = s["ix"][16:19]
    assert not tr["searched"][o1] and not tr["searched"][o3] and tr["ncand"][o0] == 1 and tr["best"][o0] == 20
    # two equal minima: the first of the visiting order wins the index; the ratio test decides by nnratio
    for name, decided in (("tie_ratio_0p9", "ratio"), ("tie_ratio_1p0", "ratio"), ("tie_ratio_1p5", "accept")):
        s = S.by_name(name)
        tr = results[name][3]
        for i in s["ix"]:
            assert (tr["decided"][i], tr["pos"][i], tr["best"][i], tr["best2"][i]) == (decided, 0, 12, 12)
        assert [int(tr["best_idx"][i]) > 2 * k for k, i in enumerate(s["ix"])] == [False, True, True]     # not the lower index


def test_rotation_scene_outcomes(results):
    def bins(name):
        s = S.by_name(name)
        n, m12, _, tr = results[name]
        assert (tr["decided"][s["ix"]] == "accept").all()
        cnt = np.bincount(tr["bin"][s["ix"]], minlength=30)
        kept = sorted({int(tr["bin"][i]) for i in s["ix"] if m12[i] >= 0})
        return cnt[cnt > 0].tolist(), kept, n
    assert bins("rot_10_1_1") == ([10, 1, 1], [2, 5, 8], 12)
    assert bins("rot_11_1_1") == ([11, 1, 1], [2], 11)
    assert bins("rot_20_2_1") == ([20, 2, 1], [2, 5], 22)
    assert bins("rot_1_1_10") == ([1, 1, 10], [2, 5, 8], 12)
    assert bins("rot_equal_bins") == ([2, 2, 2, 2], [2, 5, 8], 6)               # the lowest index takes each place
    assert bins("rot_3_3_2_2") == ([3, 2, 3, 2, 1], [1, 3, 5], 8)
    cnt, kept, n = bins("rot_half")
    assert (cnt, kept) == ([3, 4, 2, 3, 5], [0, 1, 10])
    cnt, kept, n = bins("rot_below_half")
    assert (cnt, kept) == ([2, 3, 4, 3], [1, 5, 8])
    cnt, kept, n = bins("rot_displaced")
    assert cnt == [3, 2, 2, 3] and n == 6                                        # bin 3 stays (one match), bin 2 goes
    s = S.by_name("rot_wrap")
    assert results["rot_wrap"][3]["bin"][s["ix"]].tolist() == [1, 1, 1, 1, 0, 4, 4, 6, 6, 6, 9]


def test_ladder_candidate_counts_and_positions(results):
    s = S.by_name("ladder")
    tr = results["ladder"][3]
    assert tr["ncand"][s["ix"]].tolist() == s["lad"]["counts"] == list(S.LADDER_COUNTS) * 2
    a, b = s["ix"][:10], s["ix"][10:]
    assert [int(tr["pos"][i]) for i in a[1:]] == [c - 1 for c in S.LADDER_COUNTS[1:]]       # line A: the last entry wins
    assert (tr["decided"][a[1:]] == "accept").all() and tr["skip_eq"][a].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert (tr["pos"][b[1:]] == 0).all() and tr["displaced"][b[2:]].tolist() == b[1:-1]     # line B: each takes entry 0 from the one before
    assert results["ladder"][0] == 10
    seen, owned = set(), {}
    for s in S.ladder_variants():
        name, lad = s["name"], s["lad"]
        n, m12, _, tr = results[name]
        probe = s["ix"][0]
        line = lad["line"]
        t = tr[probe]
        assert t["ncand"] == lad["count"], name
        for row, target, do in lad["owners"]:
            assert (tr["decided"][row], tr["best_idx"][row], tr["best"][row]) == ("accept", target, do), name
            assert tr["ncand"][row] == lad["count"]
        wpos = lad["wpos"]
        if not lad["owners"]:
            lo = min(wpos.values())
            first = min(p for p, w in wpos.items() if w == lo)
            assert t["pos"] == first and t["best"] == lo and t["best_idx"] == line[first], name
            others = [p for p in wpos if p != first]
            if others:
                assert t["second_pos"] == others[0] and t["best2"] == wpos[others[0]], name
                assert t["decided"] == ("ratio" if "_fail" in name else "accept"), name
                seen.add((lad["count"], first, int(np.sign(others[0] - first)) * (1 if abs(others[0] - first) == 1 else 2)))
            else:
                assert lad["count"] == 1 and t["best2"] == M.INT_MAX and t["decided"] == "accept"
        else:
            tag = name.split("_", 1)[1]
            c = lad["count"]
            want = {"win_lt": ("accept", (c - 1) // 2, 1, 0, 0), "win_eq": ("accept", (c - 1) // 2, 0, 1, 0),
                    "win_gt": ("accept", c - 1, 0, 0, 1), "second_eq": ("accept", c - 1, 0, 1, 0),
                    "second_gt": ("ratio", c - 1, 0, 0, 1)}.get(tag)
            if want is not None:
                assert (t["decided"], t["pos"], t["skip_lt"], t["skip_eq"], t["owned_gt"]) == want, name
            else:
                assert tag == "both" and t["decided"] == "accept" and t["pos"] == c - 1 and t["skip_eq"] == 1 and t["owned_gt"] >= 1
            owned.setdefault(c, set()).add(tag)
    # every length with the winner first and last, and at the positions 63 / 64 / 127 where the list reaches them; the runner-up
    # directly before (-1), directly behind (+1) and far from it (+-2)
    for c in S.LADDER_COUNTS[2:]:
        for pw in {0, c - 1} | {p for p in (63, 64, 127) if p < c}:
            rel = {r for cc, p, r in seen if (cc, p) == (c, pw)}
            assert rel & {-1, 1} and (c == 2 or rel & {-2, 2}), (c, pw, rel)
    assert all(tags == {"win_lt", "win_eq", "win_gt", "second_eq", "second_gt", "both"} for tags in owned.values())
    assert set(owned) == {2, 63, 64, 65, 127, 128, 129, 200}


def test_dependency_scenes_depend(results):
    """Taking the earlier feature out of frame 1 changes the named rows (and for the counter-cases nothing)."""
    n = 0
    for s in S.all_scenes():
        dep = s.get("dep")
        if dep is None:
            continue
        _, m12, _, tr = results[s["name"]]
        _, m12d, _, _ = M.run(s, drop=dep["drop"])
        changed = [int(i) for i in np.nonzero(m12 != m12d)[0] if i != dep["drop"]]
        if dep["changes"]:
            assert changed == sorted(dep["rows"]), (s["name"], changed)
            print("%-28s without feature %3d rows %s change: %s -> %s" % (s["name"], dep["drop"], changed, m12d[changed].tolist(),
                                                                         m12[changed].tolist()))
        else:
            assert changed == [], s["name"]
        for i, c in s.get("lad", {}).get("lists", {}).items():
            assert tr["ncand"][i] == c
        n += 1
    assert n >= 35
    for name, accepted, displaced in (("same_2_decreasing", 2, 1), ("same_2_equal", 1, 0), ("same_64_decreasing", 51, 50),
                                      ("same_64_equal", 1, 0), ("same_64_increasing", 1, 0)):
        n, m12, _, tr = results[name]
        assert ((tr["decided"] == "accept").sum(), (tr["displaced"] >= 0).sum(), n) == (accepted, displaced, 1), name
    assert results["same_64_decreasing"][1][63] == 0 and (results["same_64_equal"][1][1:] == -1).all()
    assert (results["same_64_decreasing"][3]["decided"][:13] == "th_low").all()


def test_boundary_scenes(results):
    for n1 in (1, 63, 64, 65, 128):
        s = S.by_name("n1_%d" % n1)
        assert len(s["k1"]) == n1 and results[s["name"]][0] == (1 if n1 == 1 else n1)
    for k in (0, 63, 64, 129):
        s = S.by_name("only_%d" % k)
        n, m12, _, tr = results[s["name"]]
        assert len(s["k1"]) == 130 and n == 1 and np.nonzero(tr["ncand"])[0].tolist() == [k] and m12[k] == 0


def test_lds_layout_of_the_assignment_kernel():
    """init_assign_lds and the mode choice of launch_search_for_initialization (csrc/k_guided.hip:1396-1427) restated in
    init_search_model.assign_mode: the four cap pairs of the device tests take the four layouts, and the layout changes where
    the arithmetic says it does."""
    modes = [M.assign_mode(*p)[0] for p in M.CAP_PAIRS]
    assert modes == [M.MODE_STAGED | M.MODE_DBL, M.MODE_STAGED, M.MODE_DBL, 0]
    assert all(M.assign_mode(*p)[1] <= M.LDS_BUDGET for p in M.CAP_PAIRS)
    # with cap1 == cap2 == c: staged and double-buffered up to 2048, staged up to 2865 (2866 and 2867 do not fit: the padded list
    # lengths take 2880 words), double-buffered up to 4096, neither up to 5734
    edge = {c: M.assign_mode(c, c) for c in (1, 2048, 2049, 2865, 2866, 2867, 4096, 4097, 5734, 5735)}
    assert [edge[c][0] for c in (1, 2048, 2049, 2865, 2866, 2867, 4096, 4097, 5734)] == [3, 3, 1, 1, 2, 2, 2, 0, 0]
    assert edge[5735] is None and edge[2048][1] == M.LDS_BUDGET
    assert M.assign_tables(5735, 5734) == 112 * 1024 and M.assign_mode(5735, 5734) == (0, 144 * 1024)
    assert M.assign_tables(5736, 5734) > 112 * 1024 and M.assign_mode(5736, 5734) is None
