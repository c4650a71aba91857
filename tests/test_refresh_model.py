"""The numpy model of orbhip_map_refresh (tests/refresh_model.py) on known answers, and the guard scenes the device tests rely on
(tests/test_map_refresh.py): each property is asserted to be present, so a scene that stopped discriminating fails here.  No GPU."""
import numpy as np

import refresh_model as R

f32 = np.float32
SF = R.make_scene(0, nkf=2, P=1)["sf"]


def test_one_observer_on_an_axis_gives_the_unit_normal():
    for axis in range(3):
        pos, Ow = np.zeros(3, f32), np.zeros((1, 3), f32)
        pos[axis], Ow[0, axis] = 5, 2
        n, mn, mx = R.normal_depth(pos, Ow, 0, 0, SF, 8)
        want = np.zeros(3, f32)
        want[axis] = 1
        assert R.bits(n).tobytes() == R.bits(want).tobytes()
        assert mx == f32(3) and mn == f32(f32(3) / SF[7])


def test_two_opposite_observers_give_plus_zero():
    pos = np.array([1, 2, 3], f32)
    Ow = np.array([[1, 2, 7], [1, 2, -1]], f32)
    n, _, _ = R.normal_depth(pos, Ow, 0, 0, SF, 8)
    assert R.bits(n).tolist() == [0, 0, 0]                       # +0.0f, not -0.0f


def test_levels_give_the_expected_distances():
    pos, Ow = np.array([0, 0, 4], f32), np.zeros((1, 3), f32)
    for nlevels in (1, 8, 16):
        _, mn, mx = R.normal_depth(pos, Ow, 0, 0, SF, nlevels)
        assert mx == f32(4) and mn == f32(f32(4) / SF[nlevels - 1])
        _, mn, mx = R.normal_depth(pos, Ow, 0, nlevels - 1, SF, nlevels)
        assert mx == f32(f32(4) * SF[nlevels - 1]) and mn == f32(mx / SF[nlevels - 1])
    assert SF[0] == 1 and R.normal_depth(pos, Ow, 0, 0, SF, 1)[1] == f32(4)


def test_point_at_a_camera_centre_gives_nan():
    n, _, mx = R.normal_depth(np.ones(3, f32), np.ones((1, 3), f32), 0, 0, SF, 8)
    assert np.isnan(n).all() and mx == 0


def test_distinctive_known_answers():
    z = np.zeros(32, np.uint8)
    one, two = z.copy(), z.copy()
    one[0], two[0] = 1, 3
    assert R.distinctive([z], [0]) == 0
    assert R.distinctive([z, one], [0, 0]) == 0                  # both medians 0 (N = 2 reads the self distance): the first wins
    assert R.distinctive([two, z, one], [0, 0, 0]) == 0          # distances 2, 1, 1: every median is 1, the first wins
    far = z.copy()
    far[0] = 0xFF
    assert R.distinctive([far, z, one], [0, 0, 0]) == 1          # medians 7, 1, 1: the first of the two least
    assert R.distinctive([far, z, one], [0, 1, 0]) == 0          # N = 2 reads the self distance again
    assert R.distinctive([z, one], [1, 0]) == 1 and R.distinctive([z, one], [1, 1]) == -1


def test_guard_scene_discriminates():
    cnt = R.guard_counts(R.guard_scene())
    print(cnt)
    assert all(cnt[k] >= 1 for k in "abcdefg"), cnt


def test_refresh_leaves_bad_points_and_empty_lists_alone():
    sc = R.make_scene(11, nkf=6, P=9, lengths=[3, 0, 2], bad_points=(3,))
    status, best, desc, normal, mn, mx = R.refresh(sc, 3)
    for p in (1, 3, 4, 7):
        assert status[p] == 0 and best[p] == -1
        assert desc[p].tobytes() == sc["desc"][p].tobytes() and R.bits(normal[p]).tobytes() == R.bits(sc["normal"][p]).tobytes()
        assert mn[p] == sc["min_dist"][p] and mx[p] == sc["max_dist"][p]
    assert all(status[p] == 3 for p in (0, 2, 5, 6, 8))
    assert (R.refresh(sc, 1)[0][[0, 2]] == 1).all() and (R.refresh(sc, 2)[0][[0, 2]] == 2).all()
