"""The frame grid model (tests/grid_model.py) against the CPU oracle on every constructed scene (tests/grid_scenes.py), the wrong
variants the scenes must be able to see, and the counts the scenes claim -- computed here, not trusted from the construction.
Where model and oracle disagree the reference's source decides (src/Frame.cc:574-589, :671-736)."""
import numpy as np
import pytest

import grid_model as M
import grid_scenes as S


@pytest.fixture(scope="module")
def scenes():
    return S.modelled()


def test_scene_rule_finite_and_bounded(scenes):
    for group in scenes.values():
        for s in group:
            k = s["kps"]
            assert np.isfinite(k["x"]).all() and np.isfinite(k["y"]).all(), s["name"]
            assert (np.abs(k["x"]) <= S.LIMIT).all() and (np.abs(k["y"]) <= S.LIMIT).all(), s["name"]
            assert all(np.isfinite(float(g)) and abs(float(g)) <= S.LIMIT for g in s["gp"])
            for w in s.get("windows", []):
                assert all(np.isfinite(float(v)) and abs(float(v)) <= S.LIMIT for v in w), (s["name"], w)


def test_exact_grid_cells_stated_in_the_issue():
    """x = 4 -> column 1, 12 -> 2, 20 -> 3, -3.99 -> 0; -4 and 508 fall outside."""
    col = lambda x: M.pos_in_grid(x, 0, S.EXACT)
    assert [col(4) // 48, col(12) // 48, col(20) // 48, col(-3.99) // 48] == [1, 2, 3, 0]
    assert col(-4) == -1 and col(508) == -1 and col(-0.0) == 0 and col(S.step(-4, 1)) == 0
    assert float(S.EXACT[2]) == 0.125 and float(S.EXACT[3]) == 0.125


def test_model_grid_matches_oracle(oracle, scenes):
    for group in scenes.values():
        for s in group:
            off, idx = oracle.grid_build(s["kps"], s["gp"])
            assert np.array_equal(off, s["grid"][0]) and np.array_equal(idx, s["grid"][1]), s["name"]


def test_model_windows_match_oracle(oracle, scenes):
    n = 0
    for group in ("wins", "proj", "init"):
        for s in scenes[group]:
            for w, want in zip(s["windows"], s["lists"]):
                got = oracle.features_in_area(s["kps"], s["grid"], s["gp"], float(w[0]), float(w[1]), float(w[2]), int(w[3]),
                                              int(w[4]))
                assert got.tolist() == want, (s["name"], w)
                n += 1
    assert n > 100


def test_every_wrong_variant_changes_a_scene(scenes):
    """How many scenes each variant of the model changes; every count must be at least 1."""
    changed = {v: [] for v in M.VARIANTS}
    for v in M.VARIANTS:
        for s in scenes["cells"]:
            off, idx = M.grid_build(s["kps"], s["gp"], v)
            if not (np.array_equal(off, s["grid"][0]) and np.array_equal(idx, s["grid"][1])):
                changed[v].append(s["name"])
        for group in ("wins", "proj", "init"):
            for s in scenes[group]:
                g = M.grid_build(s["kps"], s["gp"], v)
                lists = [M.features_in_area(s["kps"], g, s["gp"], *w, variant=v) for w in s["windows"]]
                if v == "no_grid":      # brute force has no visiting order: what it must not do is find other features
                    differs = any(sorted(a) != sorted(b) for a, b in zip(lists, s["lists"]))
                else:
                    differs = lists != s["lists"]
                if differs:
                    changed[v].append(s["name"])
    counts = {v: len(c) for v, c in changed.items()}
    print("scenes changed per variant:", counts)
    for v in M.VARIANTS:
        print("  %-14s %s" % (v, ", ".join(changed[v])))
    assert all(c >= 1 for c in counts.values()), counts
    # the scenes through which the matchers show the visiting order must themselves see a wrong order
    for v in ("row_major", "cell_unsorted"):
        for group in ("proj", "init"):
            assert {s["name"] for s in scenes[group]} & set(changed[v]), (v, group)


def _chunks(rec):
    return [rec[i:i + 16] for i in range(0, len(rec), 16)]


def test_claimed_window_counts_occur(scenes):
    cols, chunk_totals, cand = set(), set(), set()
    edge_empty = mid_empty = sentinel = False
    early = set()
    for s in scenes["wins"]:
        for w, lst in zip(s["windows"], s["lists"]):
            cand.add(len(lst))
            x, y, r = S.f32(w[0]), S.f32(w[1]), S.f32(w[2])
            wc = M.window_cells(s["gp"], x, y, r)
            if wc is None:
                gx, gy = (x - s["gp"][0]) * s["gp"][2], (y - s["gp"][1]) * s["gp"][3]
                rx, ry = r * s["gp"][2], r * s["gp"][3]
                early.add("x0" if gx - rx >= 64 else ("x1" if gx + rx <= -1 else ("y0" if gy - ry >= 48 else "y1")))
                assert lst == []
                continue
            cols.add(wc[1] - wc[0] + 1)
            sentinel |= wc[1] == 63 and wc[3] == 47
            rec = M.column_records(s["grid"], wc)
            ch = _chunks(rec)
            tot = [sum(c) for c in ch]
            chunk_totals.update(tot)
            edge_empty |= any(len(c) == 16 and c[0] == 0 and c[-1] == 0 and sum(c) > 0 for c in ch)
            mid_empty |= any(tot[i] == 0 and tot[i - 1] > 0 and tot[i + 1] > 0 and len(ch[i]) == 16 for i in range(1, len(ch) - 1))
    print("columns per window:", sorted(cols))
    print("records per 16-column chunk:", sorted(chunk_totals))
    print("candidates per window:", sorted(cand))
    assert cols >= {1, 15, 16, 17, 32, 33, 64}
    assert chunk_totals >= {0, 15, 16, 17, 63, 64, 65}
    assert cand >= set(S.CLUSTER_COUNTS)
    assert edge_empty and mid_empty and sentinel and early == {"x0", "x1", "y0", "y1"}
    # the level filters all occur, over octaves 0..7
    assert {(int(w[3]), int(w[4])) for s in scenes["wins"] for w in s["windows"]} >= set(S.LEVEL_FILTERS)
    assert set(np.unique(scenes["wins"][0]["kps"]["octave"])) == set(range(8))


def test_cluster_radii_give_exactly_the_claimed_counts(scenes):
    s = [s for s in scenes["wins"] if s["name"] == "cluster"][0]
    for k, lst in zip(S.CLUSTER_COUNTS, s["lists"]):          # the first windows of the scene, levels (0, 0)
        assert len(lst) == k


def test_radius_edge_features_are_on_and_one_step_inside(scenes):
    for s in scenes["wins"]:
        if not s["name"].startswith("radius_edges"):
            continue
        x, y, r = [S.f32(v) for v in s["windows"][0][:3]]
        k = s["kps"]
        dx, dy = np.abs(k["x"] - x), np.abs(k["y"] - y)
        got = set(s["lists"][0])
        inside = np.nextafter(r, S.f32(0))
        for d, o in ((dx, dy), (dy, dx)):
            on = np.nonzero((d == r) & (o < r))[0]
            just = np.nonzero((d == inside) & (o < r))[0]
            assert len(on) >= 2 and len(just) >= 1
            assert not (set(on.tolist()) & got) and set(just.tolist()) <= got
            # both ends: a feature below and one above the centre
            c, p = (x, k["x"]) if d is dx else (y, k["y"])
            assert (p[on] < c).any() and (p[on] > c).any()
        # within the radius but not in the grid is only the model's "no_grid" variant's business
        assert all(M.pos_in_grid(k["x"][i], k["y"][i], s["gp"]) >= 0 for i in got)


def test_outermost_cells_hold_passing_features(scenes):
    """Features that pass and whose column (row) is the first or the last of the floor / ceil range."""
    lo = hi = 0
    for s in scenes["wins"] + scenes["proj"]:
        for w, lst in zip(s["windows"], s["lists"]):
            wc = M.window_cells(s["gp"], w[0], w[1], w[2])
            if wc is None or wc[0] == 0 or wc[1] == 63:
                continue                          # clamped windows do not count
            cc = [M.pos_in_grid(s["kps"]["x"][i], s["kps"]["y"][i], s["gp"]) // 48 for i in lst]
            lo += wc[0] in cc
            hi += wc[1] in cc
    assert lo >= 2 and hi >= 2, (lo, hi)
    assert any(len(set(lst)) for s in scenes["wins"] if s["name"] == "outer_cells" for lst in s["lists"])


def test_outside_grid_within_radius_occurs(scenes):
    n = 0
    for s in scenes["wins"] + scenes["proj"] + scenes["init"]:
        for w, lst in zip(s["windows"], s["lists"]):
            brute = M.features_in_area(s["kps"], None, s["gp"], *w, variant="no_grid")
            n += len(set(brute) - set(lst))
            assert set(lst) <= set(brute)
    assert n >= 3


def test_claimed_cell_counts_occur(scenes):
    by = {s["name"]: s for s in scenes["cells"]}
    for m in (2, 3, 17, 200):
        off, idx = by["multi_%d" % m]["grid"]
        for c in S.EDGE_CELLS:
            e = idx[off[c]:off[c + 1]]
            assert len(e) == m, (m, c)
            assert (np.diff(e) > 0).all()
            if m >= 3:     # interleaved over the threads: neighbours in the cell are far apart in the index order
                assert len(set(e // 256)) >= 3 or m == 3 and len(set(e // 256)) >= 2
        assert idx.max() >= 2048 and (np.diff(off) == m).sum() == len(S.EDGE_CELLS)
        assert np.diff(off).max() == m
    assert sorted(len(s["kps"]) for s in scenes["cells"] if s["name"].endswith("_exact") and s["name"][0] == "n") == \
        [0, 1, 2047, 2048, 2049, 2100]
    off, idx = by["one_cell_200"]["grid"]
    assert off[-1] == 200 and np.diff(off).max() == 200 and idx.tolist() == list(range(200))
    assert by["all_outside"]["grid"][0][-1] == 0 and len(by["all_outside"]["kps"]) == 50
    for name in ("n2100_exact", "n2100_inexact"):
        off = by[name]["grid"][0]
        assert 0 < off[-1] < 2100 and np.diff(off).max() >= 3
    # the halves: in column 0 from -0.0 and from just above -0.5; 63.5 and -0.5 outside, just below 63.5 inside
    k = by["half_x_exact"]["kps"]
    cx = (k["x"] / 8).astype(np.float32)
    cell = np.array([M.pos_in_grid(k["x"][i], k["y"][i], S.EXACT) for i in range(len(k))])
    col = np.where(cell >= 0, cell // 48, -1)
    want = {-0.5: -1, float(S.step(-0.5, 1)): 0, -0.25: 0, 0.5: 1, 1.5: 2, 2.5: 3, 62.5: 63, float(S.step(63.5, -1)): 63, 63.5: -1}
    for c, w in want.items():
        assert col[cx == np.float32(c)].tolist() == [w] * int((cx == np.float32(c)).sum()) and (cx == np.float32(c)).any(), c
    assert col[(cx == 0) & np.signbit(cx)].tolist() == [0]
    k = by["half_y_exact"]["kps"]
    cy = (k["y"] / 8).astype(np.float32)
    row = np.array([M.pos_in_grid(k["x"][i], k["y"][i], S.EXACT) for i in range(len(k))])
    row = np.where(row >= 0, row % 48, -1)
    assert row[cy == np.float32(47.5)].tolist() == [-1] and row[cy == S.step(47.5, -1)].tolist() == [47]
    assert row[cy == np.float32(46.5)].tolist() == [47] and row[cy == np.float32(-0.5)].tolist() == [-1]


def test_projection_scenes_hold_the_claimed_candidates(oracle, scenes):
    """Counts and column spans as claimed; and the construction that makes the order observable does what the GPU test relies on:
    in the reference (the oracle), query i takes the i-th candidate of the model's visiting order."""
    counts, spans = set(), set()
    for s in scenes["proj"]:
        order = s["lists"][0]
        wc = M.window_cells(s["gp"], *s["window"][:3])
        assert len(order) == s["count"] and wc[1] - wc[0] + 1 == s["ncols"], s["name"]
        counts.add(len(order))
        spans.add(s["ncols"])
        for stereo in (False, True):
            c = S.proj_case(s, order, stereo)
            n, m = oracle.search_by_projection(c["kps"], c["desc"], s["gp"], c["q"], c["qd"], u_right=c["u_right"],
                                               use_ratio=False, check_ori=False)
            assert n == c["n"] and np.array_equal(m, c["match"]), (s["name"], stereo)
    assert counts >= {1, 16, 17, 32, 33} and spans >= {1, 2, 16, 17, 32, 33}
    s = [s for s in scenes["proj"] if s["name"] == "c17_n17"][0]
    ur, kept = S.stereo_u_right(s["kps"], s["lists"][0], s["window"][2])
    assert len(kept) == 15 and s["lists"][0][0] in kept and s["lists"][0][1] not in kept     # on the radius kept, a step beyond dropped
    rec = M.column_records(s["grid"], M.window_cells(s["gp"], *s["window"][:3]))
    assert sum(rec) > len(s["lists"][0])        # records that do not pass lie among the candidates


def test_initialisation_scenes_hold_the_claimed_candidates(oracle, scenes):
    got = set()
    for s in scenes["init"]:
        order = s["lists"][0]
        x, y, r = s["window"]
        wc = M.window_cells(s["gp"], x, y, r)
        assert len(order) == s["count"] and wc[1] - wc[0] + 1 == s["ncols"], s["name"]
        assert (s["kps"]["octave"][order] == 0).all() and (s["kps"]["octave"] > 0).any()
        got.add((s["ncols"], s["count"]))
        c = S.init_case(s, order)
        n, m12, prev = oracle.search_for_initialization(c["kps1"], c["d1"], c["kps2"], c["d2"], s["gp"], c["prev"],
                                                        window_size=c["window_size"], nnratio=2.0, check_ori=False)
        assert n == c["n"] and np.array_equal(m12, c["m12"]) and np.array_equal(prev, c["prev_after"]), s["name"]
    assert {c for _, c in got} == {1, 63, 64, 65, 128, 129} and {n for n, _ in got} == {1, 16, 17, 63, 64}
