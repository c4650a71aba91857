"""One more constructed edge of k_local_frustum, beside those of tests/test_localmap_edges.py: the sign of a zero Mat::dot.  A stored
normal of (0, 0, 0) under a P - Ow whose three components are negative makes every product of the dot -0.0.  Summed from 0.0, as
Mat::dot sums, the result is +0.0; summed from the first product it would be -0.0.  view_cos = dot / dist is an output of
orbhip_search_local_points and neither sign is below a viewing_cos_limit of 0, so only the bit pattern tells them apart.  One
camera, one point and a scene's handful of features."""
import numpy as np
import pytest

import localmap_model as M
import localmap_scenes as scenes
from test_localmap_gpu import FRAME, Rig, _cam_record

f32, f64 = np.float32, np.float64


def _scene(oracle):
    """Identity Rcw, tcw = 0: the point (0.1, 0.1, 2) lies in front of the camera and near the image centre; Ow = (1, 1, 4) is an
    input of its own; min / max distance 1 and 4 hold dist = 2.37."""
    sc = scenes.make(oracle, "640x480", npoints=40, nfeatures=60)
    cam = dict(sc["cam"], Rcw=np.eye(3, dtype=f32), tcw=np.zeros(3, f32), Ow=np.array([1, 1, 4], f32), viewing_cos_limit=f32(0.0))
    return dict(sc, cam=cam, keys=np.array([7919], np.uint64), pos=np.array([[0.1, 0.1, 2]], f32), normal=np.zeros((1, 3), f32),
                min_dist=np.array([1], f32), max_dist=np.array([4], f32), pdesc=sc["pdesc"][:1], flags=np.ones(1, np.uint8))


def _model_check(sc):
    """Every product of the dot is -0.0, and the model, which sums from zeros, has the point in view with view_cos = +0.0."""
    PO = sc["pos"][0] - sc["cam"]["Ow"]
    assert PO.dtype == f32 and (PO < 0).all() and all(np.signbit(f64(PO[k]) * f64(sc["normal"][0][k])) for k in range(3))
    rec, code = M.frustum(sc["cam"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    assert code[0] == M.IN_VIEW and rec["in_view"][0] == 1 and rec["view_cos"].view(np.uint32)[0] == 0
    return rec


def test_the_model_puts_the_point_in_view_with_a_positive_zero(oracle):
    _model_check(_scene(oracle))


@pytest.mark.gpu
def test_view_cos_of_three_negative_zero_products_is_positive_zero(oracle):
    sc = _scene(oracle)
    want = _model_check(sc)                                  # (on the CPU, before anything reaches the device)
    rig = Rig(sc, max_points=16)
    none = np.zeros(1, np.uint8)
    rig.compare(oracle, sc["keys"], none, 1.0, check_old_path=True)      # the whole record, n_to_match and the matches against the model
    pts, ntm = rig.lm.search(FRAME, len(sc["kps"]), _cam_record(sc["cam"], 1.0), sc["keys"], none, 0.8, sc["u_right"], sc["occupied"])[:2]
    assert ntm == 1 and pts["in_view"][0] == 1 and pts["view_cos"].view(np.uint32)[0] == 0, pts
    for f in ("u", "v", "proj_xr", "view_cos", "level", "in_view"):
        assert np.array_equal(pts[f].view(np.uint32), want[f].view(np.uint32)), f
    rig.close()
