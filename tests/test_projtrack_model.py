"""The scenes of the projection-tracking tests contain what they claim (tests/projtrack_scenes.py), by the model alone
(tests/projtrack_model.py) -- without this a device test could pass on empty results -- and the model's arithmetic is the stated
one where a coarser formulation would differ."""
import numpy as np
import pytest

import projtrack_model as PM
import projtrack_scenes as S

f32, f64 = np.float32, np.float64


def _last(oracle, sc, motion, check_ori=True):
    st = S.model_store(sc, S.stored(sc, True))
    return PM.search_last_frame(oracle, st, sc["cam"], sc["th"], sc["hold"], sc["src_kps"], motion, sc["kps"], sc["desc"], sc["gp"],
                                sc["u_right"], sc["occupied"], check_ori, sc["th_high"])


def _kf(oracle, sc, check_ori=True):
    st = S.model_store(sc, S.stored(sc, False))
    return PM.search_keyframe_points(oracle, st, sc["cam"], sc["th"], S.row_keys(sc), sc["found"], sc["src_kps"], sc["kps"], sc["desc"],
                                     sc["gp"], sc["occupied"], check_ori, sc["th_high"])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_general_scenes_hold_what_the_device_tests_rely_on(oracle, name):
    sc = S.make(oracle, name)
    assert 300 <= len(sc["kps"]) <= 900 and 300 <= len(sc["hold"]) <= 900
    for motion in ((PM.SAME,) if name == "mono" else (PM.SAME, PM.FORWARD, PM.BACKWARD)):
        q, code, qd, na, nm, match = _last(oracle, sc, motion)
        t = S.tally(code)
        print(name, "last frame, motion", motion, "active", na, "matches", nm, t)
        assert nm >= 100                                               # after the rotation check
        for rule in ("no point", "unknown", "behind", "left", "right", "top", "bottom"):
            assert t.get(rule, 0) >= 1, rule
        assert (match == -2).sum() >= 1
        assert PM.claimed_twice(oracle, q, qd, sc["kps"], sc["desc"], sc["gp"], sc["u_right"], sc["occupied"], sc["th_high"]) >= 1
        assert ((q["flags"] & 3) == 1).sum() >= 1 and ((q["flags"] & 3) == 3).sum() >= 1      # unobserved and observed points
        bad = np.array([bool(k) and not u and bool(f & 2) for k, u, f in zip(sc["hold"], sc["unknown"], sc["flags"])])
        assert (bad & (code == PM.ACTIVE)).sum() >= 1                  # a bad point takes part here
    q, code, qd, na, nm, match = _kf(oracle, sc)
    t = S.tally(code)
    print(name, "key frame", "active", na, "matches", nm, t)
    assert nm >= 100
    for rule in ("no point", "bad", "found", "left", "right", "top", "bottom", "near", "far"):
        assert t.get(rule, 0) >= 1, rule
    assert (match == -2).sum() >= 1
    # every point of this form closes the feature it takes, so no feature is ever taken twice; that two points WANT one feature
    # shows when the closing is taken away
    assert PM.claimed_twice(oracle, q, qd, sc["kps"], sc["desc"], sc["gp"], None, sc["occupied"], sc["th_high"]) == 0
    open_q = q.copy()
    open_q["flags"] &= ~2
    assert PM.claimed_twice(oracle, open_q, qd, sc["kps"], sc["desc"], sc["gp"], None, sc["occupied"], sc["th_high"]) >= 1
    levels = set(int(x) for x in q["min_level"][code == PM.ACTIVE] + 1)
    assert 0 in levels and len(sc["cam"]["scale_factors"]) - 1 in levels       # the clamp at both ends
    # a point behind the camera that projects inside the image stays active here
    st = S.model_store(sc, S.stored(sc, False))
    have = np.nonzero(code == PM.ACTIVE)[0]
    invz = PM.project(sc["cam"], np.stack([st.pts[int(S.row_keys(sc)[i])][0] for i in have]))[2]
    assert (invz < 0).sum() >= 1


def test_edge_scene_takes_every_edge(oracle):
    sc = S.edge_scene()
    ix = sc["ix"]
    lo_x, hi_x, lo_y, hi_y = S.EDGE_BOUNDS
    A = PM.ACTIVE
    want_last = dict(inside=A, u_min=A, u_max=A, v_min=A, v_max=A, u_below=PM.LEFT, u_above=PM.RIGHT, v_below=PM.TOP, v_above=PM.BOTTOM,
                     behind=PM.BEHIND, z_zero=PM.NONFINITE, nan=PM.NONFINITE, bad=A, key0=PM.NO_POINT, unknown=PM.UNKNOWN, near_on=A,
                     near_out=A, far_on=A, far_out=A, found=A)
    want_kf = dict(want_last, behind=A, bad=PM.BAD, unknown=PM.NO_POINT, near_out=PM.NEAR, far_out=PM.FAR, found=PM.FOUND)
    res = {}
    for motion in (PM.SAME, PM.FORWARD, PM.BACKWARD):
        q, code, qd, na, nm, match = res[motion] = _last(oracle, sc, motion, True)
        for case in S.EDGE_CASES:
            assert code[ix[case]] == want_last.get(case, A), case
    q, code, qd, na, nm, match = res[PM.SAME]
    assert q["u"][ix["u_min"]] == lo_x and q["u"][ix["u_max"]] == hi_x and q["v"][ix["v_min"]] == lo_y and q["v"][ix["v_max"]] == hi_y
    # one ulp outside: the model's own projection of those points
    st = S.model_store(sc, S.stored(sc, True))
    u, v, _, _ = PM.project(sc["cam"], sc["pos"])
    assert u[ix["u_below"]] == np.nextafter(lo_x, f32(-np.inf)) and u[ix["u_above"]] == np.nextafter(hi_x, f32(np.inf))
    assert v[ix["v_below"]] == np.nextafter(lo_y, f32(-np.inf)) and v[ix["v_above"]] == np.nextafter(hi_y, f32(np.inf))
    # level windows of the three motions
    o0, ot = ix["octave0"], ix["octave_top"]
    top = len(sc["cam"]["scale_factors"]) - 1
    assert (res[PM.SAME][0]["min_level"][o0], res[PM.SAME][0]["max_level"][o0]) == (-1, 1)
    assert (res[PM.FORWARD][0]["min_level"][o0], res[PM.FORWARD][0]["max_level"][o0]) == (0, -1)      # no filter at all
    assert (res[PM.BACKWARD][0]["min_level"][ot], res[PM.BACKWARD][0]["max_level"][ot]) == (0, top)
    assert (res[PM.SAME][0]["min_level"][ot], res[PM.SAME][0]["max_level"][ot]) == (top - 1, top + 1)
    assert res[PM.FORWARD][5][o0] == o0 and res[PM.BACKWARD][5][o0] == -1
    # observed against unobserved, both orders: the observed point ends up with the feature, the counts differ
    assert match[ix["obs_first"]] == ix["obs_first"] and match[ix["unobs_first"]] == ix["obs_second"]
    assert match[ix["unobs_second"]] == -1 and match[ix["obs_second"]] == -1
    # the right coordinate exactly at the radius and one float beyond
    assert match[ix["xr_inside"]] == ix["xr_inside"] and match[ix["xr_outside"]] == -1
    k = ix["xr_inside"]
    assert abs(f32(q["proj_xr"][k] - sc["u_right"][k])) <= q["radius"][k]           # the last float that passes ...
    assert abs(f32(q["proj_xr"][k] - np.nextafter(sc["u_right"][k], f32(np.inf)))) > q["radius"][k]
    k = ix["xr_outside"]
    assert abs(f32(q["proj_xr"][k] - sc["u_right"][k])) > q["radius"][k]            # ... and the first that does not
    assert abs(f32(q["proj_xr"][k] - np.nextafter(sc["u_right"][k], f32(-np.inf)))) <= q["radius"][k]
    assert match[ix["bad"]] == ix["bad"]
    # the key-frame form
    q, code, qd, na, nm, match = _kf(oracle, sc)
    for case in S.EDGE_CASES:
        assert code[ix[case]] == want_kf.get(case, A), case
    P, mn, mx = sc["pos"], sc["min_dist"], sc["max_dist"]
    for on, c, arr in (("near_on", f32(0.8), mn), ("far_on", f32(1.2), mx)):
        d = f32(np.sqrt((P[ix[on]].astype(f64) ** 2).sum()))
        assert f32(c * arr[ix[on]]) == d                               # exactly on the bound: not rejected
    d_near = f32(np.sqrt((P[ix["near_out"]].astype(f64) ** 2).sum()))
    d_far = f32(np.sqrt((P[ix["far_out"]].astype(f64) ** 2).sum()))
    # the first float whose product passes the bound
    assert f32(f32(0.8) * mn[ix["near_out"]]) > d_near and f32(f32(0.8) * np.nextafter(mn[ix["near_out"]], f32(0))) == d_near
    assert f32(f32(1.2) * mx[ix["far_out"]]) < d_far and f32(f32(1.2) * np.nextafter(mx[ix["far_out"]], f32(np.inf))) == d_far
    assert q["min_level"][ix["level_low"]] == -1 and q["max_level"][ix["level_high"]] == top + 1
    assert match[ix["behind"]] == ix["behind"] and match[ix["xr_outside"]] == ix["xr_outside"] and match[ix["found"]] == -1
    assert (q[ix["found"]].tobytes() == bytes(32)) and (q[ix["bad"]].tobytes() == bytes(32))


def test_the_reciprocal_is_a_double_division():
    """The model takes float(1.0 / double(z)) as the reference's text does (ref: src/ORBmatcher.cc:1381, :1530).  A quotient
    rounded to 53 bits and then to 24 equals the quotient rounded to 24 bits at once (53 >= 2 * 24 + 2: double rounding is
    innocuous for a division), so 1.0f / z gives the same float; the sweep pins that, and that project() is built of exactly
    these operations."""
    rng = np.random.default_rng(1)
    z = rng.uniform(0.1, 50, 200000).astype(f32)
    a = (f64(1.0) / z.astype(f64)).astype(f32)
    b = f32(1.0) / z
    assert np.array_equal(a, b)
    cam = dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), fx=f32(300), fy=f32(310), cx=f32(188), cy=f32(120),
               bounds=(f32(0), f32(376), f32(0), f32(241)))
    P = np.stack([rng.uniform(-1, 1, 1000), rng.uniform(-1, 1, 1000), rng.uniform(1, 9, 1000)], axis=1).astype(f32)
    u, v, invz, where = PM.project(cam, P)
    assert np.array_equal(invz, (1.0 / P[:, 2].astype(f64)).astype(f32))
    assert np.array_equal(u, ((f32(300) * P[:, 0]) * invz + f32(188)).astype(f32))


def test_motion_of():
    R = np.eye(3, dtype=f32)
    z = np.zeros(3, f32)
    # the current camera 0.5 in front of the last one along its axis: tcw = -0.5 z
    assert PM.motion_of(R, np.array([0, 0, -0.5], f32), R, z, 0.1, False) == PM.FORWARD
    assert PM.motion_of(R, np.array([0, 0, 0.5], f32), R, z, 0.1, False) == PM.BACKWARD
    assert PM.motion_of(R, np.array([0, 0, 0.05], f32), R, z, 0.1, False) == PM.SAME
    assert PM.motion_of(R, np.array([0, 0, -0.5], f32), R, z, 0.1, True) == PM.SAME
