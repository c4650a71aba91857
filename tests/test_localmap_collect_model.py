"""tests/localmap_collect_model.py against hand-built cases of the reference's two loops."""
import localmap_collect_model as CM


def _world():
    w = CM.World()
    for k in (11, 12, 13, 14, 15):
        w.add_point(k)
    w.put_kf(101, [11, 0, 12, 13])
    w.put_kf(102, [13, 12, 0, 14])
    w.put_kf(103, [0, 0])
    return w


def test_a_shared_point_is_kept_at_its_first_key_frame():
    w = _world()
    assert CM.collect(w, [101, 102]) == [11, 12, 13, 14]
    assert CM.collect(w, [102, 101]) == [13, 12, 14, 11]
    assert CM.collect(w, [102, 101, 102]) == [13, 12, 14, 11]
    assert CM.collect(w, [103]) == [] and CM.collect(w, []) == []


def test_a_bad_point_is_dropped_and_votes_for_nothing():
    w = _world()
    w.set_bad(12)
    assert CM.collect(w, [101, 102]) == [11, 13, 14]
    assert CM.vote(w, [12]) == []
    assert CM.vote(w, [12, 13]) == [(101, 1), (102, 1)]


def test_a_point_twice_in_the_frame_votes_twice():
    w = _world()
    assert CM.vote(w, [13, 0, 13, 11]) == [(101, 3), (102, 2)]
    assert CM.vote(w, [14, 14, 14]) == [(102, 3)]
    assert CM.vote(w, [15]) == []                      # a point no key frame observes
    assert CM.vote(w, [999]) == []                     # a point the map does not know


def test_an_empty_frame():
    w = _world()
    assert CM.vote(w, []) == [] and CM.vote(w, [0, 0, 0]) == []


def test_mutators_keep_rows_and_observations_in_step():
    w = _world()
    w.set_entry(101, 1, 14)                            # AddMapPoint
    assert CM.vote(w, [14]) == [(101, 1), (102, 1)] and CM.collect(w, [101]) == [11, 14, 12, 13]
    w.set_entry(102, 0, 0)                             # EraseMapPointMatch
    assert CM.vote(w, [13]) == [(101, 1)] and CM.collect(w, [102]) == [12, 14]
    w.erase_point(12)
    assert w.kfs[101] == [11, 14, 0, 13] and w.kfs[102] == [0, 0, 0, 14] and CM.vote(w, [12]) == []
    w.erase_kf(101)
    assert CM.vote(w, [11, 14]) == [(102, 1)]
    assert CM.skip_bytes([14, 11, 13], [13, 99]) == [0, 0, 1]
