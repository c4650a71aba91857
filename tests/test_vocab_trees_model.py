"""Irregular vocabulary trees (tests/vocab_trees.py) on the CPU: the oracle's loader and transform against the model over the
generator's node objects, the coverage that tests/test_vocab_trees_gpu.py relies on, stop words in BowVector and FeatureVector,
and the text form of such a tree through both converters."""
import numpy as np
import pytest

import vocab_trees as T

SEEDS = (101, 102, 103)
L = 4
LEVELSUP = (0, 1, 2, L, L + 2)


@pytest.fixture(scope="module", params=SEEDS)
def case(request):
    return T.tree_case(request.param, L)


def test_generated_tree_has_the_shapes_a_built_vocabulary_has(case):
    nodes = case["nodes"]
    assert 2000 < len(nodes) < 11000
    assert len(nodes[0].children) == 20                                           # two full trips of the child loop
    inner = [nd for nd in nodes[1:] if nd.children]
    assert {1, 2, 3, 9, 10, 11, 19, 20} <= set(len(nd.children) for nd in inner)
    leaves = [nd for nd in nodes[1:] if not nd.children]
    assert set(nd.depth for nd in leaves) == set(range(1, L + 1)) and max(nd.depth for nd in nodes) == L
    # ids as HKmeansStep assigns them: siblings consecutive, a parent before its children, the first child's subtree before the
    # second child's -- which is not level order: some node's first child is not the id after it in edge order
    for nd in [nodes[0]] + inner:
        assert nd.children == list(range(nd.children[0], nd.children[0] + len(nd.children))) and nd.children[0] > nd.id
    depths = [nd.depth for nd in nodes]
    assert any(depths[i] > depths[i + 1] for i in range(len(depths) - 1))       # creation order is not level order
    edge_order = [c for nd in nodes for c in nd.children]                        # the order of the device tables
    assert sorted(edge_order) == list(range(1, len(nodes)))
    assert sum(1 for e, c in enumerate(edge_order) if c != e + 1) > len(nodes) // 2
    assert [nd.word for nd in leaves] == list(range(len(leaves)))                # words in id order among the leaves ...
    by_edge = [c for c in edge_order if not nodes[c].children]
    assert sum(1 for r, c in enumerate(by_edge) if nodes[c].word != r) > len(leaves) // 2   # ... which is not edge order
    # equal siblings where the kernels split the children: across the two trips, in one slot of both, in the two columns of a quad
    def equal_at(i, j):
        return sum(1 for nd in inner if len(nd.children) > j and nodes[nd.children[i]].desc == nodes[nd.children[j]].desc)
    assert equal_at(9, 10) >= 1 and equal_at(0, 10) >= 1 and equal_at(0, 1) >= 3 and equal_at(0, 2) >= 3
    one_bit = sum(1 for nd in inner for i in nd.children for j in nd.children
                  if i < j and bin(nodes[i].desc ^ nodes[j].desc).count("1") == 1)
    assert one_bit >= 50
    w = np.array([nd.weight for nd in leaves], np.float32)
    assert (w == 0).sum() >= 0.05 * len(w) and (w < 0).sum() >= 0.02 * len(w)


def test_oracle_transform_equals_the_model_on_irregular_trees(oracle, case):
    V = oracle.Vocabulary(case["blob"])
    nodes = case["nodes"]
    assert (V.k, V.L, V.nnodes, V.nwords) == (20, L, len(nodes), sum(1 for nd in nodes[1:] if not nd.children))
    for levelsup in LEVELSUP:
        m = T.case_model(case, levelsup)
        w, wt, nid = V.transform(case["probes"], levelsup)
        assert np.array_equal(w, m["word"]) and wt.tobytes() == m["weight"].tobytes() and np.array_equal(nid, m["node"]), levelsup
    V.close()


def test_probes_reach_every_case_the_gpu_tests_rely_on(case):
    """On the model's output alone: what the device tests compare is not vacuous."""
    n = len(case["probes"])
    m = T.case_model(case, 1)
    assert (m["depth"] < L).sum() >= 0.10 * n and (m["depth"] == L).sum() >= 0.10 * n
    assert m["tie"].sum() >= 0.10 * n
    assert (m["weight"] <= 0).sum() >= 0.05 * n and (m["weight"] == 0).sum() > 0 and (m["weight"] < 0).sum() > 0
    for d in range(1, L + 1):
        assert (m["depth"] == d).sum() >= 0.02 * n, d
    assert (m["node"] == 0).sum() >= 0.10 * n and (m["node"] != 0).sum() >= 0.10 * n
    assert ((m["node"] == 0) == (m["depth"] < L - 1)).all()                      # node id 0 exactly when level L - 1 is not reached
    # neighbours in index leave the descent at different levels: the lanes of a wave diverge
    assert (m["depth"][1:] != m["depth"][:-1]).mean() > 0.8
    # the node id is not "edge index + 1", and ties are met at the positions that matter
    nodes = case["nodes"]
    edge_of = {c: e for e, c in enumerate(c for nd in nodes for c in nd.children)}
    assert sum(1 for v in m["node"] if v and edge_of[int(v)] + 1 != v) >= 0.10 * n
    m0, m4, m6 = T.case_model(case, 0), T.case_model(case, L), T.case_model(case, L + 2)
    assert (m4["node"] == 0).all() and (m6["node"] == 0).all()
    assert ((m0["node"] != 0) == (m0["depth"] == L)).all()
    for k in ("word", "weight", "depth", "tie"):
        assert np.array_equal(m0[k], m[k])


def test_ties_are_met_across_the_trips_and_the_columns(case):
    """Probes that meet equal smallest distances at children 9 and 10, 0 and 10, 0 and 1, 0 and 2 of one node exist."""
    nodes = case["nodes"]
    met = set()
    for row in case["probes"]:
        feat, cur = T._to_int(row), nodes[0]
        while cur.children:
            d = [bin(feat ^ nodes[c].desc).count("1") for c in cur.children]
            lo = min(d)
            pos = [i for i, v in enumerate(d) if v == lo]
            for pair in ((9, 10), (0, 10), (0, 1), (0, 2)):
                if pos[0] == pair[0] and pair[1] in pos:
                    met.add(pair)
            if pos[0] < 10 <= pos[-1]:
                met.add("trips")
            cur = nodes[cur.children[pos[0]]]
    assert {(0, 1), (0, 2), "trips"} <= met, met


def test_bow_and_feature_vector_leave_out_exactly_the_stopped_features(oracle, case):
    V = oracle.Vocabulary(case["blob"])
    m = T.case_model(case, 1)
    w, wt, nid = V.transform(case["probes"], 1)
    live = wt > 0
    assert 0 < (~live).sum() < len(wt)
    bw, bv = V.bow(w, wt)
    assert np.array_equal(bw, np.unique(w[live]))
    only_stopped = np.setdiff1d(w[~live], w[live])
    assert len(only_stopped) > 0 and not np.isin(only_stopped, bw).any()
    acc = {}
    for i in np.nonzero(live)[0]:
        acc[int(w[i])] = acc.get(int(w[i]), 0.0) + float(wt[i])
    norm = 0.0
    for k in sorted(acc):
        norm += abs(acc[k])
    assert np.array_equal(bv, np.array([acc[k] / norm for k in sorted(acc)]))
    ids, off, idx = oracle.feature_vector(nid, wt)
    assert sorted(idx.tolist()) == np.nonzero(live)[0].tolist()
    assert ids[0] == 0 and off[1] - off[0] == (live & (m["node"] == 0)).sum() > 0   # node 0 is a group of its own
    for g, k in enumerate(ids):
        members = idx[off[g]:off[g + 1]]
        assert (nid[members] == k).all() and (np.diff(members) > 0).all()
    V.close()


def test_text_form_of_an_irregular_tree_through_both_converters(oracle, case):
    from orbhip import distributed as D
    from orbhip.vocabulary import text_to_binary
    blob, nodes = case["blob"], case["nodes"]
    text = D.vocabulary_to_text(blob)
    ob, ow = oracle.vocabulary_text_to_blob(text)
    cb, cw = text_to_binary(text)
    assert ob == cb and np.array_equal(ow, cw)
    src, got = D.unpack_vocabulary(blob), D.unpack_vocabulary(cb)
    assert (got["k"], got["L"], got["scoring"], got["weighting"]) == (20, L, 0, 0)
    for f in ("parent", "leaf", "desc"):
        assert np.array_equal(got["nodes"][f], src["nodes"][f]), f
    assert np.array_equal(got["nodes"]["parent"], [nd.parent for nd in nodes[1:]])
    assert np.array_equal(got["nodes"]["leaf"] != 0, [not nd.children for nd in nodes[1:]])
    # six significant digits: close to the floats, zero and negative weights kept as they are
    w32 = src["nodes"]["weight"]
    assert np.allclose(cw, w32, rtol=1e-5, atol=0) and np.array_equal(cw == 0, w32 == 0) and np.array_equal(cw < 0, w32 < 0)
    assert np.array_equal(got["nodes"]["weight"], cw.astype(np.float32))
    # the double weights by word id: words are numbered in id order among the leaves
    leaf = got["nodes"]["leaf"] != 0
    by_word = cw[leaf]
    assert len(by_word) == sum(1 for nd in nodes[1:] if not nd.children)
    for nd in nodes[1::97]:
        if not nd.children:
            assert by_word[nd.word] == cw[nd.id - 1]
    V = oracle.Vocabulary(cb)
    m = T.case_model(case, 1)
    w, wt, nid = V.transform(case["probes"], 1)
    assert np.array_equal(w, m["word"]) and np.array_equal(nid, m["node"])
    bw, bv = oracle.bow_vector64(w, by_word[w], V.scoring, V.weighting)
    assert np.array_equal(bw, np.unique(w[m["weight"] > 0])) and abs(bv.sum() - 1.0) < 1e-12
    V.close()
