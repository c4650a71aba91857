"""The edge scenes of tests/test_bowseq_edges_gpu.py, validated without a device: on every pair the project's oracle equals the
definition-level model (tests/pymodels.py:search_by_bow), every deliberately wrong variant of the model is told apart on the
scenes built for it, the reach model gives every scene its target (classes, spill, the launcher's kernel), and the realised
distance tables hold the planted values.  The tallies are printed (pytest -s shows them)."""
import numpy as np
import pytest

import bowseq_edges as E

FAMILY_NAMES = sorted(E.FAMILIES)


def _same(a, b):
    return a[0] == b[0] and np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and np.array_equal(np.asarray(a[2]), np.asarray(b[2]))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_oracle_equals_model_on_every_pair(oracle, family):
    """the scene pairs and the cross pairs (2k + 1, 2k + 2) of every batch, and the frames of the lag batches"""
    pairs = 0
    for batch in E.all_batches(family):
        want = E.expected(oracle, batch)
        fr, lag = batch["frames"], batch["lag"]
        for b in range(len(fr)):
            if b < lag:
                assert want[b] is None
                continue
            got = E.model_pair(fr[b - lag], fr[b], batch["th_mode"], batch["nnratio"], batch["check_ori"], batch["use_valid"])
            assert _same(want[b], got), "%s: frame %d: the oracle and the model differ" % (batch["name"], b)
            pairs += 1
    print("%-24s pairs %d" % (family, pairs))
    assert pairs > 0


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_restated_model_equals_pymodels(family):
    """the form the variants are switched on in is the model when nothing is switched on"""
    for sc in E.scenes(family):
        assert _same(E.model(sc), E.model_pair(sc["f1"], sc["f2"], sc["th_mode"], sc["nnratio"], sc["check_ori"], sc["use_valid"],
                                               restated=True)), sc["name"]


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_realised_tables_and_reach_targets(family):
    for sc in E.scenes(family):
        # the planted distances, read back from the packed descriptors of the scene (not from the builder's bits)
        f1, f2 = sc["f1"], sc["f2"]
        for nid, want in sc["nodes"]:
            if want.size == 0:
                continue
            i1, i2 = np.nonzero(f1["node"] == np.int32(nid))[0], np.nonzero(f2["node"] == np.int32(nid))[0]
            got = E.table(f1["desc"][i1], f2["desc"][i2])
            assert got.shape == want.shape
            assert (got[want >= 0] == want[want >= 0]).all() and (got[want < 0] >= E.FAR).all(), (sc["name"], nid)
        R = E.reach(sc)
        T = sc["target"]
        for key in ("classes", "shapes", "all_fit", "tile_overflow", "byte_overflow", "kernel"):
            if key in T:
                assert R[key] == T[key], (sc["name"], key, R[key], T[key])
        # no spill unless the scene is about it: a matrix shape ('lane', 'J4', 'J8') is reached only by an item that fits, and which
        # items spill is up to the atomics
        if not T.get("all_fit", True):
            assert not R["all_fit"] and (T.get("tile_overflow") or T.get("byte_overflow") or T["shapes"] == ["coop_spill"]), sc["name"]
        else:
            assert R["all_fit"] and R["min_spill"] == 0, (sc["name"], R["bytes"], R["dcap"], R["tiles"])
        if "min_spill" in T:
            assert R["min_spill"] >= T["min_spill"] and (T["min_spill"] > 0) == (not R["all_fit"]), (sc["name"], R["min_spill"])
        if "kernel" not in T:
            assert R["kernel"] == "k_bow_lane", sc["name"]
        if "widths" in T:
            assert sorted(it["n2"] for it in R["items"]) == sorted(T["widths"])
        if T.get("full"):
            assert len(f1["desc"]) == len(f2["desc"]) == 4096 and R["NP"] == 4096 and R["lds"] <= E.LANE_LDS_LIMIT
        print("%-44s NP %4d NS %4d items %3d classes %s bytes %5d / %5d tiles %3d fit %s spill >= %d %s" % (
            sc["name"], R["NP"], R["NS"], len(R["items"]), R["classes"], R["bytes"], R["dcap"], R["tiles"], R["all_fit"],
            R["min_spill"], R["kernel"]))


def test_validity_reaches_every_code_shape_with_invalid_rows():
    """every pattern of invalid rows on a node of every code shape; the matrix shapes in scenes where every item fits in any order
    of the atomics (so steps 5a / 5b run those rows), the 258-row nodes in scenes of their own"""
    for th_mode in (0, 1):
        seen = set()
        for sc in E.scenes("validity"):
            if sc["th_mode"] != th_mode or not sc["use_valid"]:
                continue
            R = E.reach(sc)
            shape_of = {it["node"]: it["shape"] for it in R["items"]}
            f1 = sc["f1"]
            for i, tag in enumerate(f1["tag"]):
                if tag is not None and not f1["valid"][i]:
                    assert shape_of[int(f1["node"][i])] == tag[1], (sc["name"], tag)
                    if tag[1] in ("lane", "J4", "J8"):
                        assert R["all_fit"], sc["name"]
                    else:
                        assert tag[1] == "coop" or R["shapes"] == ["coop_spill"], sc["name"]
                    seen.add((tag[1], tag[2]))
        assert seen == {(s, p) for s in ("lane", "J4", "J8", "coop", "coop_spill") for p in ("first", "last", "alternate", "all")}, seen


def test_matrix_overflow_is_one_node_either_side_of_dcap():
    for sc in E.scenes("matrix_overflow"):
        R = E.reach(sc)
        over = sc["target"]["byte_overflow"]
        assert (R["bytes"] > R["dcap"]) == over and abs(R["bytes"] - R["dcap"]) < 1600 + (0 if over else 1600)
        assert (R["bytes"] - 1600 <= R["dcap"]) if over else (R["bytes"] + 1600 > R["dcap"])
    assert sorted(set(E.reach(sc)["NP"] for sc in E.scenes("matrix_overflow"))) == [512, 1024, 2048, 4096]


def test_clamp_bound_ratios_straddle_the_launchers_condition():
    at, below = E.clamp_bound_ratios()
    f32 = np.float32
    assert f32(50) < f32(at) * f32(255) and not (f32(50) < f32(below) * f32(255)) and f32(below) == np.nextafter(f32(at), f32(0))
    assert E.picks_lane_kernel(1024, at) and not E.picks_lane_kernel(1024, below)
    # below the bound the byte clamp would be wrong: 50 < r * 256 holds, 50 < r * 255 does not
    assert f32(50) < f32(below) * f32(256)


def _rows_that_differ(sc, variant):
    a, b = E.model(sc), E.model(sc, variant)
    return [i for i in range(len(a[1])) if a[1][i] != b[1][i]]


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_every_wrong_variant_is_told_apart(variant):
    total = 0
    for fam in E.VARIANT_FAMILIES[variant]:
        for sc in E.scenes(fam):
            rows = _rows_that_differ(sc, variant)
            if rows:
                print("  %-26s %-44s rows %d" % (variant, sc["name"], len(rows)))
            total += len(rows)
    print("%-26s rows that differ: %d (floor %d)" % (variant, total, E.FLOOR))
    assert total >= E.FLOOR


def test_second_best_placement_offsets_per_code_shape():
    """every listed offset the node is wide enough for, in every code shape: the planted row fails, its control matches; and the
    own-lane variants differ on every offset that is a multiple of their stride"""
    seen, told = {}, {16: set(), 64: set()}
    for sc in E.scenes("second_best_placement"):
        m = E.model(sc)
        v16, v64 = E.model(sc, "second_skips_own_lane"), E.model(sc, "second_skips_own_lane64")
        for i, tag in enumerate(sc["f1"]["tag"]):
            if tag is None:
                continue
            _, shape, off, pp, plant = tag
            assert (m[1][i] >= 0) == (not plant), (sc["name"], tag)
            seen[(shape, off)] = seen.get((shape, off), 0) + plant
            if v16[1][i] != m[1][i]:
                told[16].add((shape, off))
            if v64[1][i] != m[1][i]:
                told[64].add((shape, off))
    for shape, (nrows, n2, stride, ps) in E.PLACEMENT_SHAPES.items():
        for off in E.PLACEMENT_OFFSETS:
            if min(ps) + off < n2:
                assert seen.get((shape, off), 0) >= 1, (shape, off)
                if stride and off % stride == 0:
                    assert (shape, off) in told[stride], (shape, off, stride)
    print("planted rows per (shape, offset):", sorted(seen.items()))
    print("stride 16 told apart on:", sorted(told[16]))
    print("stride 64 told apart on:", sorted(told[64]))


def test_builder_raises_on_a_table_it_cannot_realise():
    rng = np.random.default_rng(1)
    with pytest.raises(AssertionError):
        E.build_node(rng, [(1, {0: 30}), (1, {0: 40})], 2)         # a candidate near two components
    with pytest.raises(AssertionError):
        E.build_node(rng, [(1, {0: 257})], 1)


def test_exact_ratio_pairs_and_half_rotations_exist():
    f32 = np.float32
    assert (35, 50) in E.exact_ratio_pairs(0.7)
    for r in (0.7, 0.75, 0.6, 0.9):
        ex = E.exact_ratio_pairs(r)
        assert len(ex) >= 3 and all(float(f32(r) * f32(b2)) == b1 for b1, b2 in ex)
    halves = E.half_rotations()
    print("half rotations:", halves)
    assert len(halves) >= 3 and (0, 15.0) in halves
