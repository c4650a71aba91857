"""orbhip_search_for_triangulation_sets: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-827) of one key frame against
K neighbours in one call, every key frame a resident set.  The contract is equality: row k is what the oracle and the per-pair
entry point return for neighbour k."""
import numpy as np
import pytest

import tri_sets_scene as T

pytestmark = pytest.mark.gpu

# Lower bounds per configuration and neighbour, from an oracle run on the CPU (seed 8, 593 features in key frame 1, neighbours
# of 599 / 598 / 598 / 130 features, 35 % skipped a side).  The oracle gives, after the histogram:
#   mono               118  96  84  39      (151 117 104 47 before it)
#   stereo             118  96  84  39      (151 117 104 48)
#   only_stereo         44  27  27  18      ( 56  38  35 22)
#   mono, no check_ori 151 117 104  47
AT_LEAST = {(True, False, True): (110, 90, 78, 35), (False, False, True): (110, 90, 78, 35), (False, True, True): (40, 24, 24, 15),
            (True, False, False): (140, 110, 98, 44)}
BIT_REGISTER, BIT_STRIDED = 15, 16      # orbhip_debug_path_mask: k_tri_match_sets, nodes of <= 128 / > 128 side-2 features


@pytest.fixture(scope="module")
def scene(oracle):
    S = T.build(oracle)
    S["want"] = {cfg: T.oracle_rows(oracle, S, *cfg) for cfg in T.CONFIGS}
    return S


def _matcher():
    from orbhip.extractor import ORBmatcher
    return ORBmatcher(0.6, False)


def _path_mask(reset=False):
    from orbhip import capi
    return int(capi.load().orbhip_debug_path_mask(1 if reset else 0))


def test_rows_equal_the_oracle_and_the_single_call_on_real_features(oracle, scene):
    from orbhip import guided
    S = scene
    k1, d1, g1, skip1, ur1 = S["kf1"]
    M = _matcher()
    M.put_set(1, k1, d1, g1)
    for j, nb in enumerate(S["nb"]):
        M.put_set(10 + j, nb[0], nb[1], nb[2])
    neighbours = [(10 + j, nb[3], nb[5], nb[6], nb[7]) for j, nb in enumerate(S["nb"])]
    for cfg in T.CONFIGS:
        mono, only_stereo, check_ori = cfg
        nm, m12 = guided.SearchForTriangulationSets(M._ctx, 1, skip1, neighbours, S["sf"], S["s2"],
                                                    u_right1=None if mono else ur1,
                                                    u_right2=None if mono else [nb[4] for nb in S["nb"]],
                                                    only_stereo=only_stereo, check_ori=check_ori)
        assert m12.shape == (len(S["nb"]), len(k1)) and nm.shape == (len(S["nb"]),)
        for j, (k2, d2, g2, skip2, ur2, F, exx, eyy) in enumerate(S["nb"]):
            wn, wm = S["want"][cfg][j]
            assert nm[j] == wn and np.array_equal(m12[j], wm), "neighbour %d, configuration %s" % (j, cfg)
            sn, sm = guided.SearchForTriangulation(M._ctx, k1, d1, skip1, g1, k2, d2, skip2, g2, F, exx, eyy, S["sf"], S["s2"],
                                                   u_right1=None if mono else ur1, u_right2=None if mono else ur2,
                                                   only_stereo=only_stereo, check_ori=check_ori)
            assert nm[j] == sn and np.array_equal(m12[j], sm)
            assert wn >= AT_LEAST[cfg][j]                          # not on empty work
    # the histogram has work: at least 50 matches before it on two neighbours or more, at least 10 of them removed
    before, after = [r[0] for r in S["want"][(True, False, False)]], [r[0] for r in S["want"][(True, False, True)]]
    assert sum(b >= 50 for b in before) >= 2
    assert all(b - a >= 10 for b, a in zip(before[:3], after[:3]))
    M.close()


def _hand_built(rng, sizes, nodes, order_seed):
    """Features with all-equal descriptors in nodes of the given sizes; rows a few pixels apart, three octaves; the lists of a
    node hold its features in a shuffled order (the position in the list decides, not the index)."""
    from orbhip.capi import KP_DTYPE
    n = sum(sizes)
    k = np.zeros(n, KP_DTYPE)
    k["x"] = rng.uniform(5, 300, n).astype(np.float32)
    k["y"] = rng.choice(np.array([100, 100.5, 101, 103, 110], np.float32), n)
    k["octave"] = rng.integers(0, 3, n)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    d = np.zeros((n, 32), np.uint8)
    perm = np.random.default_rng(order_seed).permutation(n).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return k, d, (np.array(nodes, np.int32), off, perm)


def test_both_kernel_paths_and_their_edges_in_one_call(oracle):
    """Side-2 nodes of 128 (the last size held in registers), 129 and 130 features against side-1 nodes of 64 (one round of the
    broadcast loop), 65 (two) and 3 features; equal descriptors, so "smallest distance, then the last position in the node's
    list" decides among the candidates near the line.  One call also holds a neighbour that shares no node, one set under two
    different F12, and key frame 1 as its own neighbour."""
    from orbhip import guided
    rng = np.random.default_rng(12)
    k1, d1, g1 = _hand_built(rng, [64, 65, 3], [10, 20, 30], 1)
    kA, dA, gA = _hand_built(rng, [128, 129, 130], [10, 20, 30], 2)
    kB, dB, gB = _hand_built(rng, [40, 50], [11, 21], 3)                     # shares no node with key frame 1
    sf = (np.float32(1.2) ** np.arange(3, dtype=np.float32)).astype(np.float32)
    s2 = (sf * sf).astype(np.float32)
    skip1 = T.flags(len(k1), 7, 0.1)
    sets = {2: (kA, dA, gA, T.flags(len(kA), 8, 0.2)), 3: (kB, dB, gB, np.zeros(len(kB), np.uint8)),
            1: (k1, d1, g1, T.flags(len(k1), 9, 0.2))}
    calls = [(2, T.F_ROWS, 900.0, 700.0), (3, T.F_ROWS, 900.0, 700.0), (2, T.F_GEN2, 150.0, 101.0), (1, T.F_ROWS, 900.0, 700.0)]
    M = _matcher()
    M.put_set(1, k1, d1, g1)
    M.put_set(2, kA, dA, gA)
    M.put_set(3, kB, dB, gB)
    _path_mask(reset=True)
    nm, m12 = guided.SearchForTriangulationSets(M._ctx, 1, skip1, [(key, sets[key][3], F, ex, ey) for key, F, ex, ey in calls], sf, s2,
                                                check_ori=False)
    mask = _path_mask()
    assert mask >> BIT_REGISTER & 1 and mask >> BIT_STRIDED & 1
    for j, (key, F, ex, ey) in enumerate(calls):
        k2, d2, g2, skip2 = sets[key]
        wn, wm = oracle.search_for_triangulation(k1, d1, skip1, g1, k2, d2, skip2, g2, F, ex, ey, sf, s2, check_ori=False)
        assert nm[j] == wn and np.array_equal(m12[j], wm), "neighbour %d" % j
    assert nm[1] == 0 and (m12[1] == -1).all()                                # no shared node
    assert nm[0] >= 100 and nm[2] >= 100 and nm[3] >= 100         # (the oracle on the CPU: 119 each)
    assert not np.array_equal(m12[0], m12[2])                     # one set, two F12: two answers
    # every node size took part: a side-1 feature of each of the three nodes found a partner in set 2
    node_of = np.empty(len(k1), np.int32)
    for g in range(3):
        node_of[g1[2][g1[1][g]:g1[1][g + 1]]] = g
    assert set(node_of[m12[0] >= 0]) == {0, 1, 2}
    # the tie rule at work: with all descriptors equal, a match is the LAST passing candidate of the node's list
    pos = np.empty(len(kA), np.int32)
    pos[gA[2]] = np.arange(len(kA))
    i1 = np.nonzero(m12[0] >= 0)[0]
    later = [(i, gA[2][p]) for i in i1[:20] for p in range(pos[m12[0][i]] + 1, gA[1][node_of[i] + 1])]
    assert len(later) > 0
    for i, i2 in later:
        off_line = (float(kA["y"][i2]) - float(k1["y"][i])) ** 2 >= 3.84 * float(s2[kA["octave"][i2]])
        assert sets[2][3][i2] or off_line
    M.close()


def test_epipole_line_and_stereo_semantics_reach_their_rows(oracle):
    """The four situations of test_oracle_tie_and_epipole_semantics as four neighbours of one call."""
    from orbhip import guided
    from orbhip.capi import KP_DTYPE
    k1 = np.zeros(2, KP_DTYPE)
    k1["x"], k1["y"] = [50, 60], [100, 100]
    k2 = np.zeros(3, KP_DTYPE)
    k2["x"], k2["y"] = [30, 40, 45], [100, 100.5, 100]
    k2b = k2.copy()
    k2b["y"][2] = 103                                          # 3 px off the line: 9 > 3.84
    d1 = np.zeros((2, 32), np.uint8)
    d2 = np.zeros((3, 32), np.uint8)
    d2[:, 0] = 0x01
    g1 = (np.array([7], np.int32), np.array([0, 2], np.int32), np.array([0, 1], np.int32))
    g2 = (np.array([7], np.int32), np.array([0, 3], np.int32), np.array([0, 1, 2], np.int32))
    sf, s2 = np.array([1.0], np.float32), np.array([1.0], np.float32)
    z2, z3 = np.zeros(2, np.uint8), np.zeros(3, np.uint8)
    mono, stereo = np.full(3, -1, np.float32), np.full(3, 5, np.float32)
    M = _matcher()
    M.put_set(1, k1, d1, g1)
    M.put_set(2, k2, d2, g2)
    M.put_set(3, k2b, d2, g2)
    cases = [(2, k2, 500.0, 400.0, mono, [2, 2]),              # equal distances: the last candidate of the node wins
             (2, k2, 47.0, 100.0, mono, [0, 0]),               # features 1 and 2 are within 10 px of the epipole
             (2, k2, 47.0, 100.0, stereo, [2, 2]),             # stereo on side 2: the epipole test does not apply
             (3, k2b, 500.0, 400.0, mono, [1, 1])]             # feature 2 is off the epipolar line
    nm, m12 = guided.SearchForTriangulationSets(M._ctx, 1, z2, [(key, z3, T.F_ROWS, ex, ey) for key, _, ex, ey, _, _ in cases], sf, s2,
                                                u_right2=[c[4] for c in cases], check_ori=False)
    for j, (key, kk, ex, ey, ur, expect) in enumerate(cases):
        wn, wm = oracle.search_for_triangulation(k1, d1, z2, g1, kk, d2, z3, g2, T.F_ROWS, ex, ey, sf, s2, u_right2=ur, check_ori=False)
        assert wm.tolist() == expect
        assert nm[j] == wn == 2 and m12[j].tolist() == expect, "neighbour %d" % j
    M.close()


def test_errors_leave_the_outputs_alone_and_the_context_usable(oracle, scene):
    from orbhip import capi, guided
    from orbhip.capi import TRI_NEIGHBOUR_DTYPE, OrbHipError, _p
    S = scene
    k1, d1, g1, skip1, _ = S["kf1"]
    k2, d2, g2, skip2, _, F, exx, eyy = S["nb"][3]
    M = _matcher()
    M.put_set(1, k1, d1, g1)
    M.put_set(2, k2, d2, g2)
    L, h = capi.load(), M._ctx.handle

    def raw(keys, nlevels=8, K=None, skip2_of=None):
        """The C entry point on sentinel-filled outputs: (return code, outputs untouched?)."""
        nb = np.zeros(len(keys), TRI_NEIGHBOUR_DTYPE)
        nb["key2"], nb["F12"], nb["ex"], nb["ey"] = keys, F.reshape(9), exx, eyy
        sk2 = np.zeros(sum(skip2_of[k] for k in keys) if skip2_of else len(keys) * len(k2), np.uint8)
        sf, s2 = np.ones(max(nlevels, 8), np.float32), np.ones(max(nlevels, 8), np.float32)
        m12 = np.full((max(len(keys), 1), len(k1)), -77, np.int32)
        nm = np.full(max(len(keys), 1), -77, np.int32)
        rc = L.orbhip_search_for_triangulation_sets(h, 1, _p(skip1), None, _p(nb), len(keys) if K is None else K, _p(sk2), None,
                                                    _p(sf), _p(s2), nlevels, 0, 0, _p(m12), _p(nm))
        return rc, bool((m12 == -77).all() and (nm == -77).all())

    assert raw([2, 999]) == (-1, True)                         # ORBHIP_E_ARG: an unknown key
    assert "unknown set" in capi.last_error(h)
    assert raw([2], nlevels=65) == (-1, True)
    assert raw([2], K=-1) == (-1, True)
    assert raw([2], nlevels=0) == (-1, True)
    kb = k2.copy()
    kb["octave"][5] = 8                                        # no such level among nlevels2 = 8
    M.put_set(3, kb, d2, g2)
    assert raw([2, 3]) == (-1, True)
    assert "octave" in capi.last_error(h)
    assert raw([2, 3], nlevels=9) == (0, False)                # the same call with a ninth level is valid
    assert raw([], K=0) == (0, True)                           # K = 0: OK, nothing written
    # more distinct keys than the limit in force: six sets are resident, then the limit drops to four
    small = {}
    for key in (4, 5, 6):
        M.put_set(key, k2[:40], d2[:40])
        small[key] = 40
    assert M.set_limit(4) == 4
    small.update({2: len(k2), 3: len(k2)})
    assert raw([2, 3, 4, 5, 6], nlevels=9, skip2_of=small) == (-1, True)
    assert "limit" in capi.last_error(h)
    assert raw([2, 4, 4, 2, 5], nlevels=9, skip2_of=small) == (0, False)     # four distinct keys with key frame 1: within it
    with pytest.raises(OrbHipError):
        guided.SearchForTriangulationSets(M._ctx, 1, skip1, [(999, skip2, F, exx, eyy)], S["sf"], S["s2"])
    # afterwards: a valid batched call and a valid single call on the same context still give the oracle's result
    wn, wm = S["want"][(True, False, True)][3]
    nm, m12 = guided.SearchForTriangulationSets(M._ctx, 1, skip1, [(2, skip2, F, exx, eyy)], S["sf"], S["s2"])
    assert nm[0] == wn and np.array_equal(m12[0], wm) and wn >= AT_LEAST[(True, False, True)][3]
    sn, sm = guided.SearchForTriangulation(M._ctx, k1, d1, skip1, g1, k2, d2, skip2, g2, F, exx, eyy, S["sf"], S["s2"])
    assert sn == wn and np.array_equal(sm, wm)
    M.close()
