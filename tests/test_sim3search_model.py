"""The model of ORBmatcher::SearchBySim3 (tests/sim3search_model.py) on the CPU: a scene worked out by hand, the constructed scenes of
tests/sim3search_scenes.py ending where they are meant to, and every named wrong variant of the model changing at least one scene --
so that tests/test_sim3search_gpu.py, which compares the device with this model on these scenes, can tell each of them apart."""
import numpy as np
import pytest

import sim3search_model as M
import sim3search_scenes as S

f32, f64 = np.float32, np.float64


def _result_key(out):
    return b"".join(a.tobytes() for a in (out["q"][0], out["q"][1], out["best"][0], out["best"][1], out["dist"][0], out["dist"][1],
                                          out["n_active"], out["match12"])) + bytes([out["nfound"] & 255])


@pytest.fixture(scope="module")
def scenes():
    return dict(edge=S.edge_scene(), assoc=S.assoc_scene()[0], agree=S.agree_scene(), same=S.same_scene(), pair=S.pair_scene(50, 40))


@pytest.fixture(scope="module")
def results(oracle, scenes):
    return {name: S.model(oracle, sc) for name, sc in scenes.items()}


def test_hand_computed_scene(oracle):
    """Both key frames at the identity, s12 = 2, R12 = I, t12 = (0.5, 0, 0): sR21 = 0.5 I, t21 = (-0.25, 0, 0).  Key frame 1's point
    Xw = (1.5, 0.5, 2) lands at p3Dc2 = (0.5, 0.25, 1): u = 64 * 0.5 + 0.5 = 32.5 and v = 16.5 with key frame 1's intrinsics (64, 64,
    0.5, 0.5) -- key frame 2's (32, 32, 0, 0) would give (16, 8).  dist3D = sqrt(1.3125); with mfMaxDistance = 1.2 * dist3D the ratio
    is 1.2 and the level ceil(log 1.2 / log 1.2) = 1 or 2 depending on logf's rounding -- so mfMaxDistance = 1.5 * dist3D:
    log 1.5 / log 1.2 = 2.22, level 3, radius = 2 * 1.2^3 = 3.456, levels [2, 3].  Key frame 2's point Xw = (0.25, 0.125, 0.5) goes to
    p3Dc1 = 2 Xw + t12 = (1, 0.25, 1): u = 64.5, v = 16.5."""
    cam1 = S.camera(np.eye(3), np.zeros(3), 64, 64, 0.5, 0.5)
    cam2 = S.camera(np.eye(3), np.zeros(3), 32, 32, 0, 0)
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    sides = [S._side(S.SET1, S.ROW1, cam1, S._kps([[64.5, 16.5]], 3), d[:1]), S._side(S.SET2, S.ROW2, cam2, S._kps([[32.5, 16.5]], 2), d[1:])]
    d3 = f32(np.sqrt(f64(1.3125)))
    d1 = f32(np.sqrt(f64(1) + f64(0.0625) + f64(1)))
    pts = [(np.uint64(11), (1.5, 0.5, 2), (0, 0, 1), d3 / f32(2), f32(1.5) * d3, S.flip(d[1], (3, 4, 5)), 1),
           (np.uint64(12), (0.25, 0.125, 0.5), (0, 0, 1), d1 / f32(2), f32(1.5) * d1, S.flip(d[0], (9,)), 1)]
    sc = S._scene(sides, [[11], [12]], 2.0, np.eye(3), (0.5, 0, 0), 2.0, pts)
    out = S.model(oracle, sc)
    sR21, t21, sR12, t12 = out["sim"]
    assert np.array_equal(sR21, 0.5 * np.eye(3, dtype=f32)) and t21.tolist() == [-0.25, 0, 0] and np.array_equal(sR12, 2 * np.eye(3, dtype=f32))
    q1, q2 = out["q"][0][0], out["q"][1][0]
    r3 = f32(f32(2.0) * (S.LS.S ** np.arange(8)).astype(f32)[3])
    assert (q1["u"], q1["v"], q1["radius"], q1["proj_xr"], q1["min_level"], q1["max_level"], q1["flags"]) == (32.5, 16.5, r3, 0, 2, 3, 3)
    assert (q2["u"], q2["v"], q2["radius"], q2["min_level"], q2["max_level"], q2["flags"]) == (64.5, 16.5, r3, 2, 3, 3)
    assert abs(float(r3) - 3.456) < 1e-6
    assert out["best"][0].tolist() == [0] and out["dist"][0].tolist() == [3] and out["best"][1].tolist() == [0] and out["dist"][1].tolist() == [1]
    assert out["match12"].tolist() == [0] and out["nfound"] == 1 and out["n_active"].tolist() == [1, 1]


def test_edge_scene_ends_where_it_is_meant_to(scenes, results):
    sc, out = scenes["edge"], results["edge"]
    code = out["code"][0]
    for case, want in S.EDGE_EXPECT.items():
        assert code[sc["ix"][case]] == want, (case, M.EXITS[code[sc["ix"][case]]])
    assert set(S.EDGE_EXPECT) == set(S.EDGE_CASES)
    assert (out["code"][1] == M.NO_POINT).all() and out["n_active"][1] == 0        # a row without a point on side 2
    # every active case finds the feature placed where it projects
    act = np.nonzero(code == M.ACTIVE)[0]
    assert np.array_equal(out["best"][0][act], act) and (out["dist"][0][act] <= 6).all()
    # the depths the issue names, as the two gemms leave them
    st = S.model_store(sc)
    sR12, sR21, t21 = M.compose(sc["s12"], sc["R12"], sc["t12"])
    z = {c: M.gemm3(sR21, M.gemm3(np.eye(3), st.pts[int(sc["keys"][sc["ix"][c]])][0], np.zeros(3)), t21)[0, 2] for c in S.EDGE_CASES if c.startswith("z_")}
    assert z["z_pzero"] == 0 and not np.signbit(z["z_pzero"]) and not np.signbit(z["z_nzero_world"])
    assert z["z_nzero"] == 0 and np.signbit(z["z_nzero"]) and z["z_neg_tiny"] == -S.TINY and z["z_pos_tiny"] == S.TINY


def test_assoc_scene_separates_the_two_associations(oracle):
    sc, ua, ub = S.assoc_scene()
    assert ua != ub and sc["sides"][1]["cam"]["bounds"][1] == max(ua, ub)
    a, b = S.model(oracle, sc), S.model(oracle, sc, "other_assoc")
    assert sorted([int(a["n_active"][0]), int(b["n_active"][0])]) == [0, 1]
    assert a["n_active"][0] == (1 if ua < ub else 0)


def test_agree_scene(scenes, results):
    sc, out = scenes["agree"], results["agree"]
    ix = sc["ix"]
    assert np.array_equal(out["match12"], sc["expect"]) and out["nfound"] == 5
    b1, e1, b2, e2 = out["best"][0], out["dist"][0], out["best"][1], out["dist"][1]
    a, b = ix["only_0"]
    assert b1[a] == b and e1[a] <= 100 and b2[b] == -1 and sc["rows"][1][b] == 0     # the best of direction 0 holds no point
    a, b = ix["only_1"]
    assert b2[b] == a and e2[b] <= 100 and b1[a] == -1
    a, b = ix["chain"]
    assert b1[a] == b and b2[b] not in (a, -1)
    (a, b), (a2, _) = ix["shared"], ix["shared_other"]
    assert b1[a] == b and b1[a2] == b and b2[b] == a
    assert e1[ix["d100"][0]] == 100 and e2[ix["d100"][1]] == 100
    assert e1[ix["d101_0"][0]] == 101 and e2[ix["d101_0"][1]] <= 100 and e2[ix["d101_1"][1]] == 101 and e1[ix["d101_1"][0]] <= 100
    assert e1[ix["d60"][0]] == 60 and e2[ix["d60"][1]] == 60
    assert out["code"][0][ix["taken1"][0]] == M.SKIPPED and out["code"][1][ix["taken2"][1]] == M.SKIPPED
    assert out["code"][0][ix["bad"][0]] == M.BAD and out["code"][0][ix["erased"][0]] == M.UNKNOWN and out["code"][0][ix["stale"][0]] == M.UNKNOWN
    a, b = ix["levels"]
    assert b1[a] == b and e1[a] == 32 and sc["sides"][1]["kps"]["octave"][ix["levels_up"][1]] == 1
    assert len(sc["rows"][0]) != len(sc["rows"][1])


def test_same_key_frame_on_both_sides(scenes, results):
    sc, out = scenes["same"], results["same"]
    has = sc["rows"][0] != 0
    assert np.array_equal(out["match12"][has], np.nonzero(has)[0]) and (out["match12"][~has] == -1).all() and out["nfound"] == has.sum() >= 20


def test_row_shapes(oracle):
    for n1, n2 in S.SIZES:
        sc = S.pair_scene(n1, n2)
        assert (len(sc["rows"][0]), len(sc["rows"][1])) == (n1, n2) == (len(sc["sides"][0]["kps"]), len(sc["sides"][1]["kps"]))
        out = S.model(oracle, sc)
        assert out["nfound"] >= 1 and out["n_active"].min() >= 1
    assert {n for s in S.SIZES for n in s} >= {1, 63, 64, 65, 255, 256, 257}
    for empty in ((True, False), (False, True), (True, True)):
        out = S.model(oracle, S.pair_scene(50, 40, empty=empty))
        assert out["nfound"] == 0 and [int(a) == 0 for a in out["n_active"]] == list(empty)


def test_pair_scene_has_matches_and_one_sided_ones(results):
    out = results["pair"]
    vn1 = np.where(out["dist"][0] <= 100, out["best"][0], -1)
    vn2 = np.where(out["dist"][1] <= 100, out["best"][1], -1)
    assert out["nfound"] >= 10 and ((vn1 >= 0) & (out["match12"] < 0)).any() and (vn2 >= 0).sum() > out["nfound"]


WHERE = dict(z_le="edge", closed_bounds="edge", other_assoc="assoc", norm_ow="edge", dst_intrinsics="edge", view_test="edge",
             levels_plus="agree", th_low="agree", lt_th_high="agree", no_agreement="agree", one_direction="agree", ignore_taken2="agree",
             stale_resolved="agree")


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_each_wrong_variant_changes_a_scene(oracle, scenes, results, variant):
    assert set(WHERE) == set(M.VARIANTS)
    name = WHERE[variant]
    wrong = S.model(oracle, scenes[name], variant)
    sc, right = scenes[name], results[name]
    if variant == "z_le":
        # z == 0 of either sign goes on to an infinite or NaN u and fails IsInImage, so `<= 0` changes where the loop leaves and
        # nothing that the call returns: the one variant no output can tell apart
        assert _result_key(wrong) == _result_key(right) and any((a != b).any() for a, b in zip(wrong["code"], right["code"]))
    else:
        assert _result_key(wrong) != _result_key(right), variant
    ix = sc["ix"]
    # ... and it changes the case that was built for it
    if variant == "z_le":
        assert wrong["code"][0][ix["z_pzero"]] == M.BEHIND and wrong["code"][0][ix["z_nzero"]] == M.BEHIND
    elif variant == "closed_bounds":
        assert wrong["code"][0][ix["u_max"]] == M.ACTIVE and wrong["code"][0][ix["v_max"]] == M.ACTIVE
    elif variant == "norm_ow":
        assert wrong["code"][0][ix["norm"]] == M.ACTIVE
    elif variant == "dst_intrinsics":
        assert wrong["code"][0][ix["quirk_in"]] == M.RIGHT and wrong["code"][0][ix["quirk_out"]] == M.ACTIVE
    elif variant == "view_test":
        assert wrong["code"][0][ix["view"]] == M.VIEW
    elif variant == "levels_plus":
        assert wrong["best"][0][ix["levels"][0]] == ix["levels_up"][1] and wrong["match12"][ix["levels"][0]] == -1
    elif variant == "th_low":
        assert wrong["match12"][ix["d60"][0]] == -1 and wrong["match12"][ix["d100"][0]] == -1
    elif variant == "lt_th_high":
        assert wrong["match12"][ix["d100"][0]] == -1 and wrong["match12"][ix["d60"][0]] >= 0
    elif variant == "no_agreement":
        assert wrong["match12"][ix["only_0"][0]] == ix["only_0"][1] and wrong["match12"][ix["chain"][0]] == ix["chain"][1]
    elif variant == "one_direction":
        assert wrong["match12"][ix["only_1"][0]] == ix["only_1"][1]
    elif variant == "ignore_taken2":
        assert wrong["match12"][ix["taken2"][0]] == ix["taken2"][1] and right["match12"][ix["taken2"][0]] == -1
    elif variant == "stale_resolved":
        assert wrong["match12"][ix["stale"][0]] == ix["stale"][1] and right["match12"][ix["stale"][0]] == -1
