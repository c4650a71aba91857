"""The native drop-in legs that take the vocabulary as a file, once more with an irregular tree (tests/vocab_trees.py), so that
ORBVocabulary::assemble and Frame::ComputeBoW meet stop words, node 0 as a group and ids in creation order.  The programs, their
inputs and every comparison are those of tests/test_gpu_dropin.py and tests/test_frame_build.py: their test functions run
unchanged, with the one call that makes their vocabulary answered by the tree made here."""
import numpy as np
import pytest

import vocab_trees as T

pytestmark = pytest.mark.gpu


def _tree_for(oracle, frame, seed, L, levelsup):
    """A tree over the frame's descriptors, with what the leg must meet asserted on the oracle's side."""
    d = oracle.Extractor(1000)(frame)[1]
    nodes, blob = T.make_tree(seed, L, pool=d)
    m = T.model_transform(nodes, L, d, levelsup)
    V = oracle.Vocabulary(blob)
    w, wt, nid = V.transform(d, levelsup)
    V.close()
    assert np.array_equal(w, m["word"]) and np.array_equal(nid, m["node"])
    assert (wt == 0).sum() > 5 and (wt < 0).sum() > 5 and (nid == 0).sum() > 20 and len(set(nid.tolist())) > 5
    return blob


def test_cpp_dropin_classes_match_oracle_on_an_irregular_tree(oracle, tmp_path, monkeypatch):
    """tests/native/test_dropin: ORBVocabulary::loadFromBinaryFile + transform(features, BowVector, FeatureVector, 4)."""
    import test_gpu_dropin as G
    from orbhip import distributed as D, synth
    blob = _tree_for(oracle, synth.make_frames(50, 752, 480, 2)[0], 401, 6, 4)       # the program's first frame
    monkeypatch.setattr(D, "make_synthetic_vocabulary", lambda *a, **kw: blob)
    G.test_cpp_dropin_classes_match_oracle(oracle, tmp_path)


def test_cpp_frame_constructor_on_an_irregular_tree(oracle, tmp_path, monkeypatch):
    """tests/native/test_frame_dropin: Frame::ComputeBoW (levelsup 4) step by step and inside the frame build."""
    import test_frame_build as G
    from orbhip import distributed as D, synth
    blob = _tree_for(oracle, synth.make_frames(45, 752, 480, 4)[0], 402, 6, 4)
    monkeypatch.setattr(D, "make_synthetic_vocabulary", lambda *a, **kw: blob)
    G.test_cpp_frame_constructor_in_one_launch(tmp_path)
