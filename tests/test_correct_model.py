"""The numpy model of orbhip_map_correct_sim3 / orbhip_map_correct_se3 (tests/correct_model.py) on known answers, against the rank rule
the device call states, and the guard scene the device tests rely on (tests/test_map_correct.py): every wrong variant is asserted to
change an output bit, so a scene that stopped discriminating fails here.  No GPU."""
import numpy as np

import correct_model as C
import refresh_model as R

f32, f64 = np.float32, np.float64
IDENT = C.sim3([0, 0, 0, 1], [0, 0, 0], 1.0)
POINTS = np.array([[1, 2, 3], [0.1, -7.3, 2.25], [1e-3, 5e4, -3.3333333], [0, 0, 0]], f32)


def xf_pair(a, b):
    x = np.zeros((), C.XF_DTYPE)
    x["Siw"], x["corrected_Swi"] = a, b
    return x


def same(a, b):
    return C.bits(a).tobytes() == C.bits(b).tobytes()


def test_identity_pair_leaves_a_position_bit_identical():
    for p in POINTS:
        assert same(C.correct_point(xf_pair(IDENT, IDENT), p), p)


def test_pure_scale_by_two():
    for p in POINTS:
        assert same(C.correct_point(xf_pair(IDENT, C.sim3([0, 0, 0, 1], [0, 0, 0], 2.0)), p), p * f32(2))


def test_quarter_turn_about_z():
    h = np.sqrt(f64(0.5))
    turn = C.sim3([0, 0, h, h], [0, 0, 0], 1.0)
    v = C.sim3_map(turn, [f64(1), f64(0), f64(0)])
    assert abs(v[0]) < 4e-16 and abs(v[1] - 1) < 4e-16 and v[2] == 0          # x -> y, to the rounding of sqrt(1/2)
    got = C.correct_point(xf_pair(turn, IDENT), np.array([3, 0, 5], f32))
    assert abs(got[0]) < 2e-15 and got[1] == f32(3) and got[2] == f32(5)
    got = C.correct_point(xf_pair(IDENT, turn), np.array([0, 2, -1], f32))
    assert got[0] == f32(-2) and abs(got[1]) < 1e-15 and got[2] == f32(-1)


def test_siw_then_its_exact_inverse_at_a_dyadic_scale():
    Siw = C.sim3([0, 0, 0, 1], [1, 2, 3], 4.0)
    Swi = C.sim3([0, 0, 0, 1], [-0.25, -0.5, -0.75], 0.25)                      # exact: every intermediate is a short dyadic number
    for p in POINTS[:2]:
        assert same(C.correct_point(xf_pair(Siw, Swi), p), p)
    inv = C.sim3_inverse(Siw)
    assert inv["s"] == 0.25 and np.array_equal(inv["t"], [-0.25, -0.5, -0.75])


def rank_rule(sc):
    """The call as include/orbhip.h states it: no sequence, an observer counts as corrected when 0 <= rank < corr."""
    P = len(sc["keys"])
    status, pos, normal = np.zeros(P, np.uint8), sc["pos"].copy(), sc["normal"].copy()
    mn, mx = sc["min_dist"].copy(), sc["max_dist"].copy()
    for p in range(P):
        if sc["flags"][p] & C.MP_BAD:
            continue
        c = sc["corr"][p]
        pos[p], status[p] = C.correct_point(sc["xf"][c], sc["pos"][p]), 1
        obs = sc["obs_kf"][sc["off"][p]:sc["off"][p + 1]]
        if len(obs):
            rank = sc["kfs"]["rank"][obs]
            Ow = np.where(((rank >= 0) & (rank < c))[:, None], sc["kfs"]["Ow_after"][obs], sc["kfs"]["Ow_before"][obs])
            normal[p], mn[p], mx[p] = R.normal_depth(pos[p], Ow, sc["ref_pos"][p], int(sc["ref_level"][p]), sc["sf"], sc["nlevels"])
            status[p] = 3
    return status, pos, normal, mn, mx


def test_the_sequence_and_the_rank_rule_agree():
    for sc in (C.guard_scene(), C.make_scene(3, nkf=20, K=1, P=40), C.make_scene(4, nkf=6, K=6, P=60, small=False)):
        a, b = C.correct_sim3(sc), rank_rule(sc)
        assert np.array_equal(a[0], b[0]) and all(same(x, y) for x, y in zip(a[1:], b[1:]))


def test_guard_scene_discriminates():
    cnt = C.guard_counts(C.guard_scene(), C.guard_se3_scene())
    print(cnt)
    assert set(cnt) == set(C.VARIANTS_SIM3) | {"float_accum"} and all(v >= 1 for v in cnt.values()), cnt
    # the centre variants must show in the normal, the arithmetic variants already in the position
    sc = C.guard_scene()
    good = C.correct_sim3(sc)
    for v in ("all_after", "all_before", "own_after"):
        other = C.correct_sim3(sc, variant=v)
        assert same(good[1], other[1]) and not same(good[2], other[2]), v
    for v in ("fused_cross", "float_maps"):
        assert not same(good[1], C.correct_sim3(sc, variant=v)[1]), v


def test_guard_seed_search_is_reproducible():
    first = next(s for s in range(8) if all(v >= 1 for v in C.guard_counts(C.guard_scene(s), C.guard_se3_scene(s)).values()))
    assert first == C.GUARD_SEED


def test_bad_points_and_empty_lists():
    sc = C.make_scene(11, nkf=6, K=3, P=9, lengths=[3, 0, 2], bad_points=(3,))
    status, pos, normal, mn, mx = C.correct_sim3(sc)
    assert status.tolist() == [3, 1, 3, 0, 1, 3, 3, 1, 3]
    assert same(pos[3], sc["pos"][3]) and not same(pos[1], sc["pos"][1])
    for p in (1, 3, 4, 7):
        assert same(normal[p], sc["normal"][p]) and mn[p] == sc["min_dist"][p] and mx[p] == sc["max_dist"][p]


def test_se3_known_answers():
    sc = C.make_se3_scene(5, K=1, P=4, mode="move")
    eye = np.eye(3, dtype=f32).ravel()
    sc["xf"]["Rcw_before"][0], sc["xf"]["Rwc"][0] = eye, eye
    sc["xf"]["tcw_before"][0], sc["xf"]["twc"][0] = [1, 2, 3], [-1, -2, -3]
    sc["pos"] = POINTS.copy()
    sc["pos"][1], sc["pos"][2] = [0.25, -7.5, 2.25], [0.5, 4, -8]
    status, pos = C.correct_se3(sc)
    assert (status == 1).all() and same(pos, sc["pos"])           # a shift and its inverse, exact for these values
    sc = C.make_se3_scene(6, K=3, P=20, mode="set", bad_points=(2,))
    status, pos = C.correct_se3(sc)
    want = sc["pos_set"].copy()
    want[2] = sc["pos"][2]
    assert status.tolist() == [1, 1, 0] + [1] * 17 and same(pos, want)
