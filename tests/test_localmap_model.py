"""The local-map search off the device: known answers of the independent model (tests/localmap_model.py) at every exit of
Frame::isInFrustum, and the threshold table that replaces logf on the device (orbhip_debug_predict_scale_table, host only) against
MapPoint::PredictScale for every float of the ratio range."""
import os
import subprocess

import numpy as np
import pytest

import localmap_model as M

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "native_localmap", "scale_table_check")


def _bits(x):
    return int(np.array([x], f32).view(np.uint32)[0])


def _next(x, n=1):
    """The float n ulps above (n < 0: below) a positive float."""
    return np.array([_bits(x) + n], np.uint32).view(f32)[0]


def _cam(th_limit=0.5):
    sf = (f32(1.2) ** np.arange(8)).astype(f32)
    return dict(Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), Ow=np.zeros(3, f32), fx=f32(512), fy=f32(256), cx=f32(320), cy=f32(240),
                mbf=f32(40), bounds=(f32(0), f32(640), f32(0), f32(480)), scale_factors=sf, log_scale_factor=f32(np.log(f32(1.2))),
                viewing_cos_limit=f32(th_limit))


def _one(cam, P, normal=None, mn=0.1, mx=100.0):
    P = np.array(P, f32)
    if normal is None:
        normal = P / np.linalg.norm(P.astype(np.float64))
    rec, code = M.frustum(cam, P[None], np.array(normal, f32)[None], [f32(mn)], [f32(mx)])
    return rec[0], int(code[0])


def test_behind_the_camera_and_the_record_of_a_point_in_view():
    cam = _cam()
    assert _one(cam, (0, 0, -1))[1] == M.BEHIND
    rec, code = _one(cam, (1, 0.5, 4), mx=8.0)
    assert code == M.IN_VIEW and rec["in_view"] == 1
    # invz = 0.25 exactly: u = 512 * 1 * 0.25 + 320, v = 256 * 0.5 * 0.25 + 240, xr = u - 40 * 0.25
    assert rec["u"] == f32(448) and rec["v"] == f32(272) and rec["proj_xr"] == f32(438)
    dist = f32(np.sqrt(np.float64(1 + 0.25 + 16)))
    assert rec["level"] == M.predict_scale(f32(8.0) / dist, cam["log_scale_factor"], 8) == 4
    # a pose: Pc = R P + t with the sum in double and one rounding
    cam2 = dict(cam, Rcw=np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32), tcw=np.array([0.5, 0, 1], f32),
                Ow=np.array([0, 0.5, -1], f32))   # Ow = -R' t
    rec2, code2 = _one(cam2, (1, 0.5, 3), normal=(0, 0, 1), mx=8.0)
    assert code2 == M.IN_VIEW and rec2["u"] == f32(320) and rec2["v"] == f32(256 * 1 * 0.25 + 240)
    assert rec2["view_cos"] == f32(4.0 / np.float64(f32(np.sqrt(np.float64(1 + 0 + 16)))))


def test_image_bounds_one_ulp_either_side():
    cam = _cam()
    # z = 1 and focal lengths that are powers of two: u = fx * x + cx exactly
    def at(u, v):
        return _one(cam, ((u - 320) / 512.0, (v - 240) / 256.0, 1.0), normal=(0, 0, 1))
    assert at(0, 240)[0]["u"] == f32(0) and at(0, 240)[1] == M.IN_VIEW          # u == mnMinX is inside
    assert at(640, 240)[0]["u"] == f32(640) and at(640, 240)[1] == M.IN_VIEW
    assert at(320, 0)[1] == M.IN_VIEW and at(320, 480)[1] == M.IN_VIEW
    for b, (lo_code, hi_code) in enumerate(((M.LEFT, M.RIGHT), (M.TOP, M.BOTTOM))):
        bounds = list(cam["bounds"])
        for side, code in ((0, lo_code), (1, hi_code)):
            # move the bound itself by one ulp around the projection of a fixed point: u = 448, v = 272
            u0 = f32(448) if b == 0 else f32(272)
            for ulps, want in ((0, M.IN_VIEW), (1 if side == 0 else -1, code)):
                bb = list(bounds)
                bb[2 * b + side] = _next(u0, ulps)
                rec, got = _one(dict(cam, bounds=tuple(bb)), (1, 0.5, 4), mx=8.0)
                assert got == want, (b, side, ulps)


def test_distance_range_and_viewing_cosine_limits():
    cam = _cam()
    P = (0, 0, 5)   # dist = 5 exactly
    # dist < 0.8f * min: 0.8f * 6.25f rounds to 5 or next to it -- take the products themselves as the thresholds
    mn_in = max(m for m in (_next(f32(6.25), k) for k in range(-4, 5)) if not f32(5) < f32(0.8) * m)
    mn_out = _next(mn_in, 1)
    assert f32(5) < f32(0.8) * mn_out
    assert _one(cam, P, mn=mn_in, mx=100)[1] == M.IN_VIEW and _one(cam, P, mn=mn_out, mx=100)[1] == M.NEAR
    mx_in = min(m for m in (_next(f32(5 / 1.2), k) for k in range(-4, 5)) if not f32(5) > f32(1.2) * m)
    mx_out = _next(mx_in, -1)
    assert _one(cam, P, mn=0.1, mx=mx_in)[1] == M.IN_VIEW and _one(cam, P, mn=0.1, mx=mx_out)[1] == M.FAR
    # viewCos = (float)(dot / dist): normal (0, 0, c) gives 5c / 5; the limit one ulp above it rejects, at it accepts
    c = f32(0.5)
    rec, code = _one(cam, P, normal=(0, 0, c))
    assert code == M.IN_VIEW and rec["view_cos"] == c
    assert _one(dict(cam, viewing_cos_limit=_next(c, 1)), P, normal=(0, 0, c))[1] == M.VIEWCOS
    assert _one(cam, P, normal=(0, 0, _next(c, -1)))[1] == M.VIEWCOS


def test_level_clamps_and_both_radii():
    cam = _cam()
    P = (0, 0, 5)
    assert _one(cam, P, mn=0.1, mx=4.5)[0]["level"] == 0                 # ratio 0.9: ceil(negative) clamped to 0
    assert _one(cam, P, mn=0.1, mx=5.0)[0]["level"] == 0                 # ratio 1: ceil(0) = 0
    assert _one(cam, P, mn=0.1, mx=_next(f32(5), 1))[0]["level"] == 1    # just above 1
    assert _one(cam, P, mn=0.1, mx=500)[0]["level"] == 7                 # ratio 100: clamped to nlevels - 1
    hi = f32(0.998)                               # (float)0.998 lies above the double 0.998
    lo = _next(hi, -1)                            # the floats either side of the double 0.998
    assert np.float64(lo) <= 0.998 < np.float64(hi)
    assert M.radius(lo, 1.0) == f32(4.0) and M.radius(hi, 1.0) == f32(2.5)
    assert M.radius(lo, 3.0) == f32(12.0) and M.radius(hi, 5.0) == f32(12.5)
    rec = np.zeros(2, M.POINT_DTYPE)
    rec[0] = (10, 20, 5, lo, 3, 1)
    q = M.queries(rec, [True, False], 3.0, cam["scale_factors"])
    assert q["radius"][0] == f32(f32(12.0) * cam["scale_factors"][3]) and (q["min_level"][0], q["max_level"][0]) == (2, 3)
    assert q["flags"][0] == 3 and q["flags"][1] == 0 and q["proj_xr"][0] == f32(5)


@pytest.mark.parametrize("s,nlevels", [(1.2, 8), (1.08, 8), (2.0, 8), (1.2, 16)])
def test_threshold_table_equals_predict_scale_for_every_float(s, nlevels):
    from orbhip import localmap
    assert os.path.exists(CHECK), "tests/native_localmap/scale_table_check is not built (make -C tests/native_localmap)"
    logS = f32(np.log(f32(s)))
    T = localmap.predict_scale_table(logS, nlevels)
    assert len(T) == nlevels - 1 and np.all(np.diff(T) > 0)
    for k in range(nlevels - 1):     # the definition, at the table's own entries
        assert M.logf(T[k]) / logS > f32(k) and not M.logf(_next(T[k], -1)) / logS > f32(k)

    def sweep(lo, hi):
        out = subprocess.check_output([CHECK, str(_bits(logS)), str(nlevels), str(_bits(lo)), str(_bits(hi))] +
                                      [str(_bits(t)) for t in T], timeout=600)
        return [int(x) for x in out.split()]
    checked, bad, trans, down = sweep(f32(0.25), f32(2.0 * float(s) ** nlevels))
    print("s=%g nlevels=%d: %d floats, %d mismatches, %d transitions, %d downward" % (s, nlevels, checked, bad, trans, down))
    assert checked > 10 ** 7 and bad == 0 and trans == nlevels - 1 and down == 0
    # ratios outside that range: tiny, huge
    for lo, hi in ((f32(1e-30), f32(1.0000001e-30)), (f32(1e-3), f32(1.001e-3)), (f32(1e6), f32(1.001e6)), (f32(3e38), f32(3.4e38))):
        assert sweep(lo, hi)[1] == 0


def test_table_builder_refuses_what_it_cannot_verify():
    from orbhip import capi, localmap
    for logS, n in ((0.0, 8), (-0.2, 8), (float("nan"), 8), (0.18, 0), (0.18, 17)):
        with pytest.raises(capi.OrbHipError):
            localmap.predict_scale_table(logS, n)
    assert len(localmap.predict_scale_table(0.18, 1)) == 0
