"""The vocabulary transform's three kernels (csrc/k_vocab.hip), the text path, BowVector / FeatureVector, orbhip_frame_build and the
batched SearchByBoW on irregular vocabulary trees (tests/vocab_trees.py): fan-outs from 1 to 20, leaves at every depth, ids in
creation order, equal siblings, stop words.  Expected values are the model's over the generator's node objects and the oracle's;
every comparison is exact.  tests/test_vocab_trees_model.py asserts, on the CPU, that the probes reach every case."""
import ctypes as C

import numpy as np
import pytest

import vocab_trees as T

pytestmark = pytest.mark.gpu

L = 4
SEEDS = (101, 102, 103)
LEVELSUP = (0, 1, 2, L, L + 2)
POISON = 0xAB
POISON32 = int(np.frombuffer(bytes([POISON] * 4), np.int32)[0])
W, H, NF, B = 640, 480, 1000, 4
# Half of the smallest match count the oracle gives over the three frame pairs of bow_scene at nnratio 0.7, by th_mode
# (th_mode 0: 388, 439, 422 matches; th_mode 1: 359, 390, 367)
MATCH_FLOOR = {0: 194, 1: 179}


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(NF, max_w=W, max_h=H, max_batch=B)
    yield e
    e.close()


@pytest.fixture(scope="module", params=SEEDS)
def case(request):
    return T.tree_case(request.param, L)


def _load(ex, blob):
    from orbhip.vocabulary import ORBVocabulary
    voc = ORBVocabulary(ex)
    voc.loadFromBinaryBlob(blob)
    return voc


def _same(got, m, idx=None, what=""):
    w, wt, nid = got
    sel = slice(None) if idx is None else idx
    assert np.array_equal(w, m["word"][sel]), "word ids differ " + what
    assert np.asarray(wt, np.float32).tobytes() == m["weight"][sel].tobytes(), "weights differ " + what
    assert np.array_equal(nid, m["node"][sel]), "node ids differ " + what


# ---- k_vocab_transform<true>: n <= 16384 ----
def test_eager_kernel_equals_model_and_oracle(oracle, ex, case):
    voc = _load(ex, case["blob"])
    V = oracle.Vocabulary(case["blob"])
    assert (voc.k, voc.L, voc.nnodes, voc.nwords) == (20, L, len(case["nodes"]), V.nwords) == (V.k, V.L, V.nnodes, V.nwords)
    probes = case["probes"]
    for levelsup in LEVELSUP:
        m = T.case_model(case, levelsup)
        for n in (1, 63, 64, 65, 1200):
            got = voc.transform_raw(probes[:n], levelsup)
            _same(got, m, slice(0, n), "(levelsup %d, n %d)" % (levelsup, n))
        rw, rwt, rnid = V.transform(probes, levelsup)
        assert np.array_equal(got[0], rw) and got[1].tobytes() == rwt.tobytes() and np.array_equal(got[2], rnid)
    V.close()


def test_eager_kernel_at_the_last_n_it_takes(ex, case):
    voc = _load(ex, case["blob"])
    n = 16384
    idx = np.arange(n) % len(case["probes"])
    _same(voc.transform_raw(case["probes"][idx], 1), T.case_model(case, 1), idx, "(n 16384)")


# ---- k_vocab_transform_quad: n > 16384 without a device count ----
@pytest.mark.parametrize("n", [16385, 16447])
def test_quad_kernel_equals_model_and_leaves_the_slack_alone(ex, case, n):
    """16385: the last workgroup holds one live quad and a tail that repeats the last descriptor and stores nothing; 16447: not a
    multiple of 64.  Host form and device form, into poisoned buffers longer than n."""
    import hiprt
    from orbhip.capi import _p, check
    _load(ex, case["blob"])
    lib = ex._L
    idx = (np.arange(n) * 7 + 3) % len(case["probes"])           # (7 and 1200 are coprime: every probe, neighbours of other depths)
    desc = np.ascontiguousarray(case["probes"][idx])
    slack = 70
    for levelsup in (1, 0, L + 2):
        m = T.case_model(case, levelsup)
        w, nid = np.full(n + slack, POISON32, np.int32), np.full(n + slack, POISON32, np.int32)
        wt = np.full(n + slack, POISON32, np.int32).view(np.float32)
        check(lib.orbhip_vocab_transform(ex.handle, _p(desc), n, levelsup, _p(w), _p(wt), _p(nid)), ex.handle, "orbhip_vocab_transform")
        _same((w[:n], wt[:n], nid[:n]), m, idx, "(host form, levelsup %d)" % levelsup)
        assert (w[n:] == POISON32).all() and (wt[n:].view(np.int32) == POISON32).all() and (nid[n:] == POISON32).all()
    m = T.case_model(case, 1)
    d_desc = hiprt.DevBuf.from_numpy(desc)
    outs = [hiprt.DevBuf.from_numpy(np.full(n + slack, POISON32, np.int32)) for _ in range(3)]
    check(lib.orbhip_vocab_transform_device(ex.handle, d_desc.ptr, n, 1, outs[0].ptr, outs[1].ptr, outs[2].ptr), ex.handle,
          "orbhip_vocab_transform_device")
    ex.sync()
    w, wt, nid = (o.to_numpy(np.int32, (n + slack,)) for o in outs)
    _same((w[:n], wt[:n].view(np.float32), nid[:n]), m, idx, "(device form)")
    assert (w[n:] == POISON32).all() and (wt[n:] == POISON32).all() and (nid[n:] == POISON32).all()
    for b in [d_desc] + outs:
        b.free()


# ---- the text path and the host mirror's BowVector / FeatureVector ----
def test_text_loaded_irregular_tree(oracle, ex, case):
    from orbhip import distributed as D
    from orbhip.vocabulary import ORBVocabulary
    text = D.vocabulary_to_text(case["blob"])
    voc = ORBVocabulary(ex)
    assert voc.loadFromText(text) and (voc.k, voc.L, voc.nnodes) == (20, L, len(case["nodes"]))
    m = T.case_model(case, 1)
    w, wt, nid = voc.transform_raw(case["probes"], 1)
    assert np.array_equal(w, m["word"]) and np.array_equal(nid, m["node"])
    ob, ow = oracle.vocabulary_text_to_blob(text)
    leaf = np.frombuffer(ob, D.VOC_NODE_DTYPE, offset=24)["leaf"] != 0
    w64 = ow[leaf][m["word"]]
    assert np.array_equal(wt, w64.astype(np.float32))
    (bw, bv), fv = voc.transform(case["probes"], 1)
    obw, obv = oracle.bow_vector64(m["word"], w64, 0, 0)
    assert np.array_equal(bw, obw) and np.array_equal(bv, obv)
    assert all(np.array_equal(a, b) for a, b in zip(fv, oracle.feature_vector(m["node"], w64)))


def test_bow_vector_and_feature_vector_drop_stop_words(oracle, ex, case):
    voc = _load(ex, case["blob"])
    V = oracle.Vocabulary(case["blob"])
    for levelsup in (1, 0, L):
        m = T.case_model(case, levelsup)
        (bw, bv), fv = voc.transform(case["probes"], levelsup)
        obw, obv = V.bow(m["word"], m["weight"])
        assert np.array_equal(bw, obw) and np.array_equal(bv, obv)
        ofv = oracle.feature_vector(m["node"], m["weight"])
        assert all(np.array_equal(a, b) for a, b in zip(fv, ofv))
        stopped = np.nonzero(m["weight"] <= 0)[0]
        assert len(stopped) > 0 and not np.isin(stopped, fv[2]).any() and len(fv[2]) == len(m["word"]) - len(stopped)
        assert not np.isin(np.setdiff1d(m["word"][stopped], m["word"][m["weight"] > 0]), bw).any()
    fv = voc.transform(case["probes"], 1)[1]
    m = T.case_model(case, 1)
    assert fv[0][0] == 0 and fv[1][1] == ((m["node"] == 0) & (m["weight"] > 0)).sum() > 0     # node 0 is a group at levelsup 1
    V.close()


# ---- orbhip_frame_build: the transform inside the captured graph, on a real frame's descriptors ----
@pytest.fixture(scope="module")
def frame_scene(oracle):
    from orbhip import synth
    img = synth.make_frames(41, W, H, 1)[0]
    k, d = oracle.Extractor(NF)(img)
    nodes, blob = T.make_tree(201, L, pool=d)
    return dict(img=img, desc=d, nodes=nodes, blob=blob)


def test_frame_build_on_an_irregular_tree(oracle, ex, frame_scene):
    s = frame_scene
    _load(ex, s["blob"])
    V = oracle.Vocabulary(s["blob"])
    rw, rwt, rnid = V.transform(s["desc"], 1)
    m = T.model_transform(s["nodes"], L, s["desc"], 1)
    assert np.array_equal(rw, m["word"]) and np.array_equal(rnid, m["node"])
    n = len(rw)
    assert (m["depth"] <= 2).sum() >= 0.05 * n and (m["depth"] == L).sum() >= 0.05 * n      # shallow and deepest leaves
    assert (rnid == 0).sum() >= 0.05 * n and (rnid != 0).sum() >= 0.05 * n and (rwt <= 0).sum() > 0
    for call in ("capture", "replay"):
        r = ex.frame_build(s["img"], levelsup=1)
        assert np.array_equal(r["desc"], s["desc"]), call
        assert np.array_equal(r["word_id"], rw) and np.array_equal(r["node_id"], rnid), call
        assert r["weight"].tobytes() == rwt.tobytes(), call
    V.close()


def test_frame_build_with_more_than_16384_slots(oracle, frame_scene):
    """k_vocab_transform<false>: a context whose frame block holds more than 16384 features runs the transform of
    orbhip_frame_build with the count on the device and n above the eager kernel's range."""
    from orbhip.extractor import ORBextractor
    s = frame_scene
    e = ORBextractor(17000, max_w=W, max_h=H)
    try:
        assert e.cap > 16384
        _load(e, s["blob"])
        V = oracle.Vocabulary(s["blob"])
        for call in ("capture", "replay"):
            r = e.frame_build(s["img"], levelsup=1)
            n = len(r["desc"])
            assert n > 1000
            m = T.model_transform(s["nodes"], L, r["desc"], 1) if call == "capture" else m
            assert (m["depth"] <= 2).sum() > 50 and (m["depth"] == L).sum() > 50 and m["tie"].sum() > 50
            _same((r["word_id"], r["weight"], r["node_id"]), m, None, "(%s)" % call)
        rw, rwt, rnid = V.transform(r["desc"], 1)
        assert np.array_equal(rw, m["word"]) and np.array_equal(rnid, m["node"])
        V.close()
    finally:
        e.close()


# ---- batched SearchByBoW: stop words and node 0 in both matchers ----
def bow_scene(oracle):
    """Four frames, the oracle's features, a tree whose descriptors come from them, the oracle's transform at levelsup 1."""
    from orbhip import synth
    frames = synth.make_frames(70, W, H, B)
    refx = oracle.Extractor(NF)
    kd = [refx(f) for f in frames]
    nodes, blob = T.make_tree(301, L, pool=np.concatenate([d for _, d in kd]))
    V = oracle.Vocabulary(blob)
    feats = []
    for k, d in kd:
        w, wt, nid = V.transform(d, 1)
        feats.append(dict(k=k, d=d, wt=wt, nid=nid, fv=oracle.feature_vector(nid, wt)))
    V.close()
    valid = (np.random.default_rng(72).random((B, 4096)) < 0.85).astype(np.uint8)      # "has a good MapPoint", by slot
    return dict(frames=frames, blob=blob, feats=feats, valid=valid)


@pytest.fixture(scope="module")
def bow(oracle):
    s = bow_scene(oracle)
    for b in range(1, B):                                        # what the pairs must contain, on the oracle's side
        f1, f2 = s["feats"][b - 1], s["feats"][b]
        assert (f1["wt"] == 0).sum() > 5 and (f1["wt"] < 0).sum() > 5 and (f2["wt"] <= 0).sum() > 10
        ids, off, _ = f2["fv"]
        sizes = np.diff(off)
        assert ids[0] == 0 and sizes[0] > 128                     # group 0: more side-2 features than k_bow_lane's largest class
        assert f1["fv"][0][0] == 0 and (sizes[1:] <= 16).sum() > 10 and (np.diff(f1["fv"][1])[1:] <= 16).sum() > 10
    return s


@pytest.mark.parametrize("th_mode", [0, 1])
def test_batched_search_by_bow_on_an_irregular_tree(oracle, ex, bow, th_mode):
    """The flow of test_hip_batched_search_by_bow_matches_oracle.  nnratio 0.7 takes k_bow_lane, 0.19 takes k_bow_seq."""
    import hiprt
    from orbhip.capi import check
    _load(ex, bow["blob"])
    feats = bow["feats"]
    cap, lib = ex.cap, ex._L
    d_img = hiprt.DevBuf.from_numpy(bow["frames"])
    d_kps, d_desc, d_cnt = hiprt.DevBuf(B * cap * 28), hiprt.DevBuf(B * cap * 32), hiprt.DevBuf(B * 4)
    d_word, d_wt, d_node = hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * cap * 4)
    d_m12, d_m21, d_nm = hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * 4)
    valid = np.ascontiguousarray(bow["valid"][:, :cap])
    d_valid = hiprt.DevBuf.from_numpy(valid)
    ex.extract_batch_device(d_img.ptr, B, W, H, W, H * W, d_kps.ptr, d_desc.ptr, cap, d_cnt.ptr)
    check(lib.orbhip_vocab_transform_device(ex.handle, d_desc.ptr, B * cap, 1, d_word.ptr, d_wt.ptr, d_node.ptr), ex.handle)
    ex.sync()
    cnt = d_cnt.to_numpy(np.int32, (B,))
    wt, node = d_wt.to_numpy(np.float32, (B, cap)), d_node.to_numpy(np.int32, (B, cap))
    for b in range(B):
        n = len(feats[b]["k"])
        assert cnt[b] == n and wt[b, :n].tobytes() == feats[b]["wt"].tobytes() and np.array_equal(node[b, :n], feats[b]["nid"])
    differs_without_stop = False
    for nnratio in (0.7, 0.19):
        check(lib.orbhip_search_by_bow_seq_device(ex.handle, d_desc.ptr, d_kps.ptr, d_cnt.ptr, d_node.ptr, d_wt.ptr, d_valid.ptr, cap,
                                                  B, 1, th_mode, C.c_float(nnratio), 1, d_m12.ptr, d_m21.ptr, d_nm.ptr), ex.handle,
              "search_by_bow_seq")
        ex.sync()
        m12, m21 = d_m12.to_numpy(np.int32, (B, cap)), d_m21.to_numpy(np.int32, (B, cap))
        nm = d_nm.to_numpy(np.int32, (B,))
        assert nm[0] == 0 and (m12[0] == -1).all() and (m21[0] == -1).all()
        for b in range(1, B):
            f1, f2 = feats[b - 1], feats[b]
            n1, n2 = len(f1["k"]), len(f2["k"])

            def ref(fv1, fv2):
                return oracle.search_by_bow(f1["d"], valid[b - 1, :n1], f1["k"]["angle"], fv1, f2["d"],
                                            valid[b, :n2] if th_mode else None, f2["k"]["angle"], fv2, th=50, th_mode=th_mode,
                                            nnratio=nnratio, check_ori=True)
            wn, w12, w21 = ref(f1["fv"], f2["fv"])
            # what a matcher that kept the words of weight 0 (w >= 0) would return: it must differ somewhere, or the pairs say
            # nothing about the stop words
            keep0 = [oracle.feature_vector(f["nid"], np.where(f["wt"] == 0, 1, f["wt"])) for f in (f1, f2)]
            differs_without_stop |= not np.array_equal(ref(keep0[0], f2["fv"])[1], w12)
            assert nm[b] == wn
            if nnratio > 0.5:
                assert wn > MATCH_FLOOR[th_mode]
            assert np.array_equal(m12[b, :n1], w12) and (m12[b, n1:] == -1).all()
            assert np.array_equal(m21[b, :n2], w21) and (m21[b, n2:] == -1).all()
            stopped1, stopped2 = np.nonzero(f1["wt"] <= 0)[0], np.nonzero(f2["wt"] <= 0)[0]
            assert (w12[stopped1] == -1).all() and (w21[stopped2] == -1).all()
        if nnratio < 0.5:
            assert differs_without_stop, "no pair in which a word of weight 0 would have matched under k_bow_seq"
        differs_without_stop = False
    for x in (d_img, d_kps, d_desc, d_cnt, d_word, d_wt, d_node, d_m12, d_m21, d_nm, d_valid):
        x.free()

