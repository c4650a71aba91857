"""The edge scenes of tests/test_localmap_edges.py, validated without a device: every case gets the exit code or level the builder
(tests/localmap_edges.py) meant for it and every tally reaches its floor, by the model alone; and the level of every threshold
case against the definition in tests/native_localmap/scale_table_check.c, ceilf(logf(r) / logS) clamped."""
import os
import subprocess

import numpy as np

import localmap_edges as edges
import localmap_model as M

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native_localmap", "scale_table_check")
_cache = {}


def _scene(oracle):
    if "sc" not in _cache:
        _cache["sc"] = edges.make(oracle)
    return _cache["sc"]


def _bits(x):
    return int(np.array([x], f32).view(np.uint32)[0])


def test_every_edge_case_hits_its_target_in_the_model(oracle):
    sc = _scene(oracle)
    tally = edges.verify(oracle, sc)
    for (kind, side), n in sorted(tally.items()):
        print("%-22s %-18s %d" % (kind, side, n))
    print("refused shapes:", sc["refused"] or "none", "| reach:", sc["reach"])
    assert edges.BASE_SHAPE in sc["shapes"]
    assert len(sc["keys"]) <= 1600 and len(sc["kps"]) <= 1100 and len(sc["rows"]) <= 3 * 32
    # the edge values are what they claim to be: on the bound, one ulp inside, one ulp outside
    model = edges.model_all(oracle, sc)
    for kind, side, cid, idx, code, lv in sc["cases"]:
        cam = sc["cams"][cid][0]
        rec0 = model["base"][0]
        if kind in edges.BOUNDS:
            b = edges.BOUNDS.index(kind)
            val, bound = rec0["u" if b < 2 else "v"][idx], f32(cam["bounds"][b])
            lower = b % 2 == 0
            want = {"at": val, "inside": edges.up(val, -1 if lower else 1), "outside": edges.up(val, 1 if lower else -1)}[side]
            assert _bits(bound) == _bits(want)
        elif kind == "limit":
            val = rec0["view_cos"][idx]
            assert _bits(cam["viewing_cos_limit"]) == _bits({"at": val, "inside": edges.up(val, -1), "outside": edges.up(val, 1)}[side])
        elif kind == "0.998":
            assert _bits(rec0["view_cos"][idx]) == _bits(f32(0.998)) + {"at": 0, "below": -1, "above": 1}[side]
        elif kind in ("near", "far"):
            d = edges.dist_of(cam, sc["pos"][idx])[0][0]
            p = f32(0.8) * sc["min_dist"][idx] if kind == "near" else f32(1.2) * sc["max_dist"][idx]
            assert (p == d) if side == "at" else (p != d)
            rejected = d < p if kind == "near" else d > p
            assert rejected == (side == "outside") and (code != M.IN_VIEW) == rejected


def test_threshold_cases_against_the_definition_of_predict_scale(oracle):
    """ratio == T[k] has level k + 1 and the ratio just below has level k, for every k of every shape: the model (libm logf through
    ctypes), the table (count of T[k] <= ratio) and scale_table_check's own ceilf(logf(r) / logS) agree on each distinct ratio."""
    assert os.path.exists(CHECK), "tests/native_localmap/scale_table_check is not built (make -C tests/native_localmap)"
    sc = _scene(oracle)
    model = edges.model_all(oracle, sc)
    seen = set()
    per_shape = {}
    for kind, side, cid, idx, code, lv in sc["cases"]:
        if kind not in ("level", "clamp") or cid == "base":
            continue
        cam, th, shape = sc["cams"][cid]
        T, logS = sc["tables"][shape], cam["log_scale_factor"]
        ratio = sc["max_dist"][idx] / edges.dist_of(cam, sc["pos"][idx])[0][0]
        assert ratio.dtype == f32
        if kind == "level":
            k = lv - 1 if side == "at" else lv
            assert (ratio == T[k]) if side == "at" else (ratio < T[k] and ratio >= edges.up(T[k], -3))
        by_table = int((ratio >= T).sum())
        assert model[cid][0]["level"][idx] == by_table == lv == M.predict_scale(ratio, logS, shape[1])
        if (shape, _bits(ratio)) in seen:
            continue
        seen.add((shape, _bits(ratio)))
        # one float: "checked mismatches transitions downward" = 1 0 0 0 when the table's level is the definition's
        out = subprocess.check_output([CHECK, str(_bits(logS)), str(shape[1]), str(_bits(ratio)), str(_bits(ratio))] +
                                      [str(_bits(t)) for t in T], timeout=60)
        assert [int(x) for x in out.split()] == [1, 0, 0, 0], (shape, float(ratio), out)
        if kind == "level" and side == "at":       # and the definition steps exactly there: the float below T[k] is one level lower
            out = subprocess.check_output([CHECK, str(_bits(logS)), str(shape[1]), str(_bits(ratio) - 1), str(_bits(ratio))] +
                                          [str(_bits(t)) for t in T], timeout=60)
            assert [int(x) for x in out.split()] == [2, 0, 1, 0], (shape, float(ratio), out)
        per_shape[shape] = per_shape.get(shape, 0) + 1
    print("distinct ratios checked per shape:", per_shape)
    for shape in sc["shapes"]:
        assert per_shape.get(shape, 0) >= (2 * (shape[1] - 1) if shape[1] > 1 else 1), shape
