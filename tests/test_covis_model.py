"""The model of the covisibility graph (tests/covis_model.py) against a brute-force set intersection and on the cases the rules
turn on: the threshold, the fall-back to the single maximum, the tie orders, AddConnection's weak links and the parent."""
import numpy as np

import covis_model as GM
import localmap_collect_model as CM


def _world(shares, extra=0):
    """Key frames 10, 20, ... ; shares = {(a, b): n}: n points of their own for every pair, plus `extra` private points each."""
    w = CM.World()
    rows, key = {}, 1000
    for (a, b), n in sorted(shares.items()):
        for _ in range(n):
            w.add_point(key)
            rows.setdefault(a, []).append(key)
            rows.setdefault(b, []).append(key)
            key += 1
    for kf in sorted(rows):
        for _ in range(extra):
            w.add_point(key)
            rows[kf].append(key)
            key += 1
    for kf in sorted(rows):
        w.put_kf(kf, rows[kf])
    return w


def _random_world(seed=5, nkf=12, npts=160):
    rng = np.random.default_rng(seed)
    w = CM.World()
    keys = [int(k) for k in (np.arange(npts) + 1) * 7]
    for k in keys:
        w.add_point(k, rng.random() < 0.1)
    for i in range(nkf):
        row = rng.choice(keys, int(rng.integers(0, 90)), replace=False)
        row[rng.random(len(row)) < 0.15] = 0
        w.put_kf((i + 1) * 3, row)
    w.erase_point(keys[4])
    w.erase_kf(9)
    w.put_kf(9, [])
    return w


def test_counter_equals_set_intersection_and_is_symmetric():
    w = _random_world()
    total = 0
    for kf in w.kfs:
        cnt = GM.counter(w, kf)
        assert cnt == GM.brute_weights(w, kf)
        assert all(k != kf for k, _ in cnt)
        for k, n in cnt:
            assert dict(GM.counter(w, k))[kf] == n
        total += len(cnt)
    assert total > 60 and GM.counter(w, 9) == []


def test_threshold_14_15_16():
    w = _world({(10, 20): 14, (10, 30): 15, (10, 40): 16})
    g = GM.Graph(root_key=10)
    GM.update_connections(w, g, 10)
    n = g.node(10)
    assert n.weights == {20: 14, 30: 15, 40: 16}
    assert n.ordered == [40, 30] and n.ordered_w == [16, 15]
    assert g.node(20).weights == {} and g.node(30).weights == {10: 15} and g.node(40).ordered == [10]
    # alone below the threshold, the link of 14 is the maximum and is taken
    GM.update_connections(w, g, 20)
    assert g.node(20).ordered == [10] and g.node(20).ordered_w == [14] and g.node(10).weights[20] == 14


def test_no_link_reaches_th_the_lower_key_of_two_maxima_wins():
    w = _world({(50, 20): 7, (50, 30): 7, (50, 40): 3})
    g = GM.Graph()
    GM.update_connections(w, g, 50)
    assert g.node(50).weights == {20: 7, 30: 7, 40: 3}
    assert g.node(50).ordered == [20] and g.node(50).ordered_w == [7]
    assert g.node(20).weights == {50: 7} and g.node(30).weights == {} and g.node(40).weights == {}
    assert g.node(50).parent == 20 and g.node(20).children == {50}


def test_ties_at_or_above_th_come_in_descending_key_order():
    w = _world({(50, 20): 15, (50, 30): 15, (50, 40): 15, (50, 60): 20, (50, 70): 14})
    g = GM.Graph()
    GM.update_connections(w, g, 50)
    assert g.node(50).ordered == [60, 40, 30, 20] and g.node(50).ordered_w == [20, 15, 15, 15]
    assert GM.covis(w, [50])[0] == ([20, 30, 40, 60, 70], [15, 15, 15, 20, 14], [60, 40, 30, 20])


def test_add_connection_lists_weak_links_in_the_neighbour():
    w = _world({(20, 30): 16, (20, 40): 16})
    g = GM.Graph()
    GM.update_connections(w, g, 20)
    assert g.node(20).ordered == [40, 30] and g.node(20).weights == {30: 16, 40: 16}
    w.put_kf(10, [0, 0, 0])                    # a new key frame that observes three of 20's points
    for i, key in enumerate(w.kfs[20][:3]):
        w.set_entry(10, i, key)
    GM.update_connections(w, g, 10)            # 10's only link is below th: it is the maximum, and 20 hears of it
    assert g.node(10).ordered == [20] and g.node(10).ordered_w == [3]
    assert g.node(20).weights == {30: 16, 40: 16, 10: 3}
    assert g.node(20).ordered == [40, 30, 10] and g.node(20).ordered_w == [16, 16, 3]
    GM.update_connections(w, g, 20)            # 20's own update lists the links >= th alone, and keeps the weight
    assert g.node(20).ordered == [40, 30] and g.node(20).weights == {10: 3, 30: 16, 40: 16}
    # the same weight again changes nothing (AddConnection returns before UpdateBestCovisibles)
    g.node(30).ordered = ["kept"]
    GM.add_connection(g, 30, 20, 16)
    assert g.node(30).ordered == ["kept"]


def test_parent_is_set_once_and_never_for_the_first_key_frame():
    w = _world({(10, 20): 16, (20, 30): 15})
    g = GM.Graph(root_key=10)
    GM.update_connections(w, g, 10)
    assert g.node(10).parent is None and g.node(10).first
    GM.update_connections(w, g, 20)
    assert g.node(20).parent == 10 and g.node(10).children == {20} and not g.node(20).first
    for i in range(5):                         # 30 becomes 20's best neighbour: the parent stays
        w.add_point(5000 + i)
        w.kfs[20].append(0), w.kfs[30].append(0)
        w.set_entry(20, len(w.kfs[20]) - 1, 5000 + i)
        w.set_entry(30, len(w.kfs[30]) - 1, 5000 + i)
    GM.update_connections(w, g, 20)
    assert g.node(20).ordered == [30, 10] and g.node(20).parent == 10 and g.node(30).children == set()


def test_a_key_frame_that_shares_nothing_is_left_alone():
    w = _world({(10, 20): 16})
    w.put_kf(30, [])
    g = GM.Graph()
    g.node(30).weights, g.node(30).ordered = {99: 1}, [99]
    GM.update_connections(w, g, 30)
    assert g.node(30).weights == {99: 1} and g.node(30).ordered == [99] and g.node(30).first
    assert GM.covis(w, [30, 10]) == [([], [], []), ([20], [16], [20])]
