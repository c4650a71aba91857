"""Known answers, computed by hand, for the model the device and the drop-in are compared with (tests/cull_model.py)."""
import cull_model as UM
import localmap_collect_model as CM


def _world(n_points, rows, levels=None):
    w, lv = CM.World(), UM.Levels()
    for p in range(1, n_points + 1):
        w.add_point(p)
    for kf, row in rows.items():
        w.put_kf(kf, row)
        lv.put(kf, (levels or {}).get(kf, [UM.level_byte(0)] * len(row)))
    return w, lv


def test_nine_tenths_of_ten():
    assert not UM.is_redundant(10, 9)            # 9 > 9.0 is false
    assert UM.is_redundant(10, 10)
    assert not UM.is_redundant(20, 18) and UM.is_redundant(20, 19)
    assert not UM.is_redundant(0, 0)             # nMPs == 0: 0 > 0.0 is false


def test_ten_points_nine_or_ten_redundant():
    # key frame 2 sees points 1..10; 3, 4, 5 see 1..9, and point 10 as well in the second world
    for last, want in ((9, (10, 9)), (10, (10, 10))):
        seen = list(range(1, last + 1))
        w, lv = _world(10, {2: list(range(1, 11)), 3: seen, 4: seen, 5: seen})
        counts, red, states = UM.cull(w, lv, [2], True)
        assert counts == [want] and red == [want[1] == 10]
        assert states[0] == [2] * last + [1] * (10 - last)


def test_a_key_frame_without_points():
    w, lv = _world(3, {2: [0, 0, 0], 3: [1, 2, 3]})
    w.set_bad(1)
    assert UM.cull(w, lv, [2, 3], True) == ([(0, 0), (2, 0)], [False, False], [[0, 0, 0], [0, 1, 1]])


def test_observations_and_others_are_different_numbers():
    # two stereo observers: Observations() is 4 but there is one other observer
    stereo = [UM.level_byte(0, stereo=True)]
    w, lv = _world(1, {2: [1], 3: [1]}, {2: stereo, 3: stereo})
    assert UM.cull(w, lv, [2], True)[0] == [(1, 0)]
    # four monocular observers: Observations() 4 > 3, three others
    w, lv = _world(1, {2: [1], 3: [1], 4: [1], 5: [1]})
    assert UM.cull(w, lv, [2], True)[0] == [(1, 1)]
    # three others but coarser than l + 1
    w, lv = _world(1, {2: [1], 3: [1], 4: [1], 5: [1]}, {3: [UM.level_byte(1)], 4: [UM.level_byte(1)], 5: [UM.level_byte(2)]})
    assert UM.cull(w, lv, [2], True)[0] == [(1, 0)]


def test_far_points_count_only_for_a_monocular_map():
    far = [UM.level_byte(0, far=True)]
    w, lv = _world(1, {2: [1], 3: [1], 4: [1], 5: [1]}, {2: far})
    assert UM.cull(w, lv, [2], False)[0] == [(0, 0)] and UM.cull(w, lv, [2], True)[0] == [(1, 1)]
    assert UM.cull(w, lv, [3], False)[0] == [(1, 1)]         # the far observation of 2 is still an observation


def test_scene_a_a_cull_takes_the_third_observer():
    w, lv, cands = UM.scene_a()
    assert UM.cull(w, lv, cands, True)[1] == [True, True]    # one batch at the start would cull both
    assert UM.sequential(w, lv, cands, True) == [2]
    assert UM.count(w, lv, 3, True)[:2] == (10, 0) and sorted(w.kfs) == [3, 4, 5]
    assert not any(p["bad"] for p in w.points.values())


def test_scene_b_a_cull_turns_points_bad():
    w, lv, cands = UM.scene_b()
    counts, red, _ = UM.cull(w, lv, cands, True)
    assert counts == [(22, 20), (12, 10)] and red == [True, False]   # one batch at the start would keep B
    assert UM.sequential(w, lv, cands, True) == [2, 3]
    assert [k for k, p in w.points.items() if p["bad"]] == [31, 32] and w.kfs[7] == [0, 0]


def test_the_root_and_skipped_key_frames_stay():
    w, lv, _ = UM.scene_a()
    w.put_kf(1, list(range(1, 11)))
    lv.put(1, [UM.level_byte(0)] * 10)
    assert UM.sequential(w, lv, [1, 2, 3, 4, 5], True, skip=lambda kf: kf == 2) == [3, 4]   # obs 5, 4; then 3 is not > 3
