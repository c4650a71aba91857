"""The batched SearchByBoW (orbhip_search_by_bow_seq_device: k_bow_lane, k_bow_seq<true / false>; csrc/k_bowseq.hip) on the edge
scenes of tests/bowseq_edges.py: every class boundary, the tile-list and byte-matrix overflows at each NP, the second best in
the winner's own lane, the comparison edges and the 255 clamp at the launcher's bound, skipped rows, stopped features, node ids
at the ends of their range, ComputeThreeMaxima's ties and cuts, and the argument edges -- bit for bit against the oracle, twice
(the ranks inside a class come from atomics).  tests/test_bowseq_edges_model.py shows on the CPU that each scene holds its edge."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bowseq_edges as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILY_NAMES = sorted(E.FAMILIES)
SENTINEL = -77


class Rig:
    def __init__(self):
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.ex = ORBextractor(50, max_w=128, max_h=128, nlevels=1)
        self.matchers = {}
        self.ORBmatcher = ORBmatcher

    def matcher(self, nnratio, check_ori):
        key = (nnratio, check_ori)
        if key not in self.matchers:
            self.matchers[key] = self.ORBmatcher(nnratio, bool(check_ori), ctx=self.ex)
        return self.matchers[key]

    def close(self):
        self.ex.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _path_mask(reset=False):
    from orbhip import capi
    return int(capi.load().orbhip_debug_path_mask(1 if reset else 0))


def _upload(batch):
    import hiprt
    from orbhip.capi import KP_DTYPE
    B, cap = len(batch["frames"]), batch["cap"]
    kps = np.zeros((B, cap), KP_DTYPE)
    kps["angle"] = batch["angle"]
    bufs = {"desc": hiprt.DevBuf.from_numpy(batch["desc"]), "kps": hiprt.DevBuf.from_numpy(kps),
            "cnt": hiprt.DevBuf.from_numpy(batch["counts"]), "node": hiprt.DevBuf.from_numpy(batch["node"]),
            "wt": hiprt.DevBuf.from_numpy(batch["wt"]), "m12": hiprt.DevBuf(B * cap * 4), "m21": hiprt.DevBuf(B * cap * 4),
            "nm": hiprt.DevBuf(B * 4)}
    if batch["use_valid"]:
        bufs["valid"] = hiprt.DevBuf.from_numpy(batch["valid"])
    return bufs


def _call(ex, bufs, cap, B, lag, th_mode, nnratio, check_ori, **over):
    a = {"desc": bufs["desc"].ptr, "kps": bufs["kps"].ptr, "cnt": bufs["cnt"].ptr, "node": bufs["node"].ptr, "wt": bufs["wt"].ptr,
         "valid": bufs["valid"].ptr if "valid" in bufs else None, "m12": bufs["m12"].ptr, "m21": bufs["m21"].ptr, "nm": bufs["nm"].ptr}
    a.update(over)
    return ex._L.orbhip_search_by_bow_seq_device(ex.handle, a["desc"], a["kps"], a["cnt"], a["node"], a["wt"], a["valid"], cap, B, lag,
                                                 th_mode, C.c_float(nnratio), check_ori, a["m12"], a["m21"], a["nm"])


def _run(ex, bufs, batch):
    from orbhip.capi import check
    B, cap = len(batch["frames"]), batch["cap"]
    check(_call(ex, bufs, cap, B, batch["lag"], batch["th_mode"], batch["nnratio"], batch["check_ori"]), ex.handle, "search_by_bow_seq")
    ex.sync()
    return (bufs["m12"].to_numpy(np.int32, (B, cap)), bufs["m21"].to_numpy(np.int32, (B, cap)), bufs["nm"].to_numpy(np.int32, (B,)))


def _want_kernel_bits(batch):
    if os.environ.get("ORBHIP_BOW_LANE", "1") == "0" or not E.picks_lane_kernel(batch["cap"], batch["nnratio"]):
        if os.environ.get("ORBHIP_BOW_GLOBAL_DESC", "0") != "0":
            return 1 << 10
        NP = E.lane_lds(batch["cap"])[0]
        full = ((NP * 36 + NP // 32 * 12 + 15) & ~15) + 64 + batch["cap"] * 64
        return 1 << (9 if full <= 150 * 1024 else 10)
    return 1 << 8


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_scene_batches_match_the_oracle_twice(oracle, rig, family):
    ex = rig.ex
    pairs = 0
    for batch in E.all_batches(family):
        want = E.expected(oracle, batch)
        bufs = _upload(batch)
        B, cap, lag = len(batch["frames"]), batch["cap"], batch["lag"]
        _path_mask(reset=True)
        got = _run(ex, bufs, batch)
        mask = _path_mask()
        assert mask & (7 << 8) == _want_kernel_bits(batch), (batch["name"], hex(mask))
        again = _run(ex, bufs, batch)
        for x in bufs.values():
            x.free()
        m12, m21, nm = got
        for b in range(B):
            if b < lag:
                assert nm[b] == 0 and (m12[b] == -1).all() and (m21[b] == -1).all(), "%s: frame %d has no predecessor" % (batch["name"], b)
                continue
            wn, w12, w21 = want[b]
            n1, n2 = len(w12), len(w21)
            bad = [i for i in range(n1) if m12[b, i] != w12[i]]
            assert nm[b] == wn and not bad and np.array_equal(m21[b, :n2], w21), \
                "%s: frame %d (%s): matches %d, the oracle %d; first rows that differ %s" % (
                    batch["name"], b, batch["scenes"][b // 2] if b % 2 and b // 2 < len(batch["scenes"]) else "cross pair",
                    nm[b], wn, [(i, batch["frames"][b - lag]["tag"][i], int(m12[b, i]), int(w12[i])) for i in bad[:6]])
            assert (m12[b, n1:] == -1).all() and (m21[b, n2:] == -1).all(), "%s: frame %d: slots beyond the counts" % (batch["name"], b)
            pairs += 1
        for g, a in zip(got, again):
            assert np.array_equal(g, a), "%s: the second run differs from the first" % batch["name"]
    assert pairs > 0
    print("%s: %d pairs" % (family, pairs))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_single_pair_entry_points_on_the_scene_pairs(oracle, rig, family):
    """ORBmatcher.SearchByBoW (k_bow_match) and SearchByBoW_sets on the scene pairs, as CSR FeatureVectors"""
    from orbhip.capi import KP_DTYPE
    n = 0
    for sc in E.scenes(family):
        f1, f2 = sc["f1"], sc["f2"]
        n1, n2 = len(f1["desc"]), len(f2["desc"])
        if n1 == 0 or n2 == 0:
            continue
        want = E.oracle_pair(oracle, f1, f2, sc["th_mode"], sc["nnratio"], sc["check_ori"], sc["use_valid"])
        m = rig.matcher(sc["nnratio"], sc["check_ori"])
        v1 = f1["valid"] if sc["use_valid"] else np.ones(n1, np.uint8)
        v2 = f2["valid"] if (sc["use_valid"] and sc["th_mode"]) else None
        g1, g2 = oracle.feature_vector(f1["node"], f1["wt"]), oracle.feature_vector(f2["node"], f2["wt"])
        got = m.SearchByBoW(f1["desc"], v1, f1["angle"], g1, f2["desc"], v2, f2["angle"], g2, kf_kf=bool(sc["th_mode"]))
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), "SearchByBoW: " + sc["name"]
        if len(g1[0]) and len(g2[0]):
            k1, k2 = np.zeros(n1, KP_DTYPE), np.zeros(n2, KP_DTYPE)
            k1["angle"], k2["angle"] = f1["angle"], f2["angle"]
            m.put_set(0x6b01, k1, f1["desc"], g1)
            m.put_set(0x6b02, k2, f2["desc"], g2)
            got = m.SearchByBoW_sets(0x6b01, v1, n1, 0x6b02, v2, n2, kf_kf=bool(sc["th_mode"]))
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), "SearchByBoW_sets: " + sc["name"]
        n += 1
    assert n > 0


def test_refused_calls_leave_the_outputs_untouched(rig):
    import hiprt
    from orbhip import capi
    ex = rig.ex
    batch = E.all_batches("node_ids")[0]
    bufs = _upload(batch)
    B, cap = len(batch["frames"]), batch["cap"]
    big = 4097
    fill12 = hiprt.DevBuf.from_numpy(np.full(B * big, SENTINEL, np.int32))
    fill21 = hiprt.DevBuf.from_numpy(np.full(B * big, SENTINEL, np.int32))
    fillnm = hiprt.DevBuf.from_numpy(np.full(B, SENTINEL, np.int32))
    out = {"m12": fill12.ptr, "m21": fill21.ptr, "nm": fillnm.ptr}
    E_ARG, E_SIZE = -1, -2                                          # include/orbhip.h
    # (4097 slots: refused on its size before any buffer is read)
    assert _call(ex, bufs, big, B, 1, 0, 0.7, 1, **out) == E_SIZE
    assert _call(ex, bufs, cap, B, -1, 0, 0.7, 1, **out) == E_ARG
    assert _call(ex, bufs, cap, 0, 1, 0, 0.7, 1, **out) == E_ARG
    for name in ("m12", "m21", "nm"):
        assert _call(ex, bufs, cap, B, 1, 0, 0.7, 1, **dict(out, **{name: None})) == E_ARG
    ex.sync()
    for x, n in ((fill12, B * big), (fill21, B * big), (fillnm, B)):
        assert (x.to_numpy(np.int32, (n,)) == SENTINEL).all()
    # and the context still works
    check_batch = _run(ex, bufs, batch)
    assert check_batch[2][1] > 0
    for x in list(bufs.values()) + [fill12, fill21, fillnm]:
        x.free()


@pytest.mark.parametrize("env", [{"ORBHIP_BOW_LANE": "0"}, {"ORBHIP_BOW_LANE": "0", "ORBHIP_BOW_GLOBAL_DESC": "1"}],
                         ids=["k_bow_seq-lds", "k_bow_seq-global"])
def test_wave_per_node_kernels_on_the_same_scenes(env):
    """k_bow_seq<true> and k_bow_seq<false> (the ablation library, a fresh child process) give the oracle's answers on every scene"""
    target = "%s::test_scene_batches_match_the_oracle_twice" % os.path.abspath(__file__)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", target], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "%d passed" % len(FAMILY_NAMES) in p.stdout, p.stdout[-1500:]
