"""SearchForInitialization on the device (k_init_cands, k_init_assign) on the constructed scenes of tests/init_search_scenes.py.
Every comparison is exact: nmatches, vnMatches12 and the bytes of the updated vbPrevMatched.  The expected values come from the
model (tests/init_search_model.py; tests/test_init_search_model.py holds it against the CPU oracle, shows which wrong
implementations the scenes can see and what each scene contains) -- never from the device.  The oracle is a second witness.

Which test reaches which code:
  sorted lists, the lane walk, commit masks       test_host_entry_every_scene (lists of 1 .. 64 entries, the dependency scenes)
  unsorted lists (65 .. 128), the rescan (129+)   the ladder scenes of the same test
  the four LDS layouts of k_init_assign           test_device_entry_at_the_four_layouts (caps of init_search_model.CAP_PAIRS)
  per-pair counts in a batch                      test_batched_pairs
  the largest caps the API takes                  test_largest_caps
  the list limits moved to 1 and to 64 / 64       test_list_limits_moved (ORBHIP_INIT_K = 1 and 64, one child process each)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import init_search_model as M
import init_search_scenes as S

pytestmark = pytest.mark.gpu

NCELL = 64 * 48
E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from orbhip.extractor import ORBextractor
    ex = ORBextractor(500, max_w=320, max_h=240)
    yield ex
    ex.close()


_EXPECTED = {}


def _expected(s):
    """(first call, second call with the first call's vbPrevMatched) by the model, computed once per scene."""
    if s["name"] not in _EXPECTED:
        first = M.run(s)[:3]
        second = M.search(s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], first[2], s["window"], s["nnratio"], s["check_ori"])[:3]
        _EXPECTED[s["name"]] = (first, second)
    return _EXPECTED[s["name"]]


def _same(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()


def _host(ctx, s, prev=None):
    from orbhip import guided
    return guided.SearchForInitialization(ctx, s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], s["prev"] if prev is None else prev,
                                          s["window"], s["nnratio"], s["check_ori"])


def _rows(s, got, want):
    bad = np.nonzero(np.asarray(got[1]) != np.asarray(want[1]))[0].tolist()
    return "%s: nmatches %d (want %d), rows that differ %s" % (s["name"], got[0], want[0], bad[:12])


def test_host_entry_every_scene(ctx, oracle):
    for s in S.all_scenes():
        first, second = _expected(s)
        got = _host(ctx, s)
        assert _same(got, first), _rows(s, got, first)
        ref = oracle.search_for_initialization(s["k1"], s["d1"], s["k2"], s["d2"], s["gp"], s["prev"], s["window"], s["nnratio"],
                                               s["check_ori"])
        assert _same(ref, first), s["name"]
        # the initialiser calls it again on the next frame with the updated vbPrevMatched
        again = _host(ctx, s, got[2])
        assert _same(again, second), _rows(s, again, second)


class _DeviceCall:
    """orbhip_grid_build_device + orbhip_search_for_initialization_device on B pairs in buffers of cap1 / cap2 slots.  The slots
    beyond a pair's counts hold usable features (level 0, inside the grid, a vbPrevMatched with candidates): a kernel that read
    them would match them."""

    def __init__(self, ctx, B, cap1, cap2):
        import hiprt
        self.ctx, self.B, self.cap1, self.cap2 = ctx, B, cap1, cap2
        self.bufs = dict(k1=hiprt.DevBuf(B * cap1 * 28), d1=hiprt.DevBuf(B * cap1 * 32), c1=hiprt.DevBuf(B * 4),
                         k2=hiprt.DevBuf(B * cap2 * 28), d2=hiprt.DevBuf(B * cap2 * 32), c2=hiprt.DevBuf(B * 4),
                         prev=hiprt.DevBuf(B * cap1 * 8), off=hiprt.DevBuf(B * (NCELL + 1) * 4), idx=hiprt.DevBuf(B * cap2 * 4),
                         m=hiprt.DevBuf(B * cap1 * 4), nm=hiprt.DevBuf(B * 4))

    def _put(self, name, a):
        import hiprt
        a = np.ascontiguousarray(a)
        assert a.nbytes <= max(self.bufs[name].nbytes, 16)
        assert hiprt.rt().hipMemcpy(self.bufs[name].ptr, a.ctypes.data, a.nbytes, 1) == 0

    def fill(self, pairs, counts=None):
        B, cap1, cap2 = self.B, self.cap1, self.cap2
        assert len(pairs) == B
        k1, k2 = np.zeros((B, cap1), S.KP_DTYPE), np.zeros((B, cap2), S.KP_DTYPE)
        d1, d2 = np.zeros((B, cap1, 32), np.uint8), np.zeros((B, cap2, 32), np.uint8)
        prev = np.zeros((B, cap1, 2), np.float32)
        c1, c2 = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b, s in enumerate(pairs):
            n1, n2 = (len(s["k1"]), len(s["k2"])) if counts is None else counts[b]
            assert n1 <= min(cap1, len(s["k1"])) and n2 <= min(cap2, len(s["k2"]))
            c1[b], c2[b] = n1, n2
            # beyond the counts: the scene's own features again (as many as there are), then copies of its first ones
            src1 = np.arange(cap1) % max(len(s["k1"]), 1)
            src2 = np.arange(cap2) % max(len(s["k2"]), 1)
            k1[b], d1[b], prev[b] = s["k1"][src1], s["d1"][src1], s["prev"][src1]
            k2[b], d2[b] = s["k2"][src2], s["d2"][src2]
        self.prev_in = prev
        for name, a in (("k1", k1), ("d1", d1), ("c1", c1), ("k2", k2), ("d2", d2), ("c2", c2), ("prev", prev),
                        ("m", np.full((B, cap1), 0x5A5A5A5A, np.int32)), ("nm", np.full(B, 0x5A5A5A5A, np.int32))):
            self._put(name, a)
        return c1, c2

    def grid(self, gp):
        from orbhip import capi
        d = self.bufs
        capi.check(capi.load().orbhip_grid_build_device(self.ctx.handle, d["k2"].ptr, d["c2"].ptr, self.cap2, self.B, gp[0], gp[1],
                                                         gp[2], gp[3], d["off"].ptr, d["idx"].ptr), self.ctx.handle, "grid_build_device")

    def search(self, gp, window, nnratio, check_ori, cap1=None):
        """The return code of orbhip_search_for_initialization_device (cap1: what the call is told, for the refused caps)."""
        from orbhip import capi
        d = self.bufs
        return capi.load().orbhip_search_for_initialization_device(
            self.ctx.handle, d["k1"].ptr, d["d1"].ptr, d["c1"].ptr, self.cap1 if cap1 is None else cap1, d["k2"].ptr, d["d2"].ptr,
            d["c2"].ptr, self.cap2, self.B, gp[0], gp[1], gp[2], gp[3], d["off"].ptr, d["idx"].ptr, d["prev"].ptr, int(window),
            nnratio, 1 if check_ori else 0, d["m"].ptr, d["nm"].ptr)

    def results(self):
        self.ctx.sync()
        d = self.bufs
        return (d["nm"].to_numpy(np.int32, (self.B,)), d["m"].to_numpy(np.int32, (self.B, self.cap1)),
                d["prev"].to_numpy(np.float32, (self.B, self.cap1, 2)))

    def run(self, pairs, counts=None):
        from orbhip import capi
        s = pairs[0]
        assert all((p["window"], p["nnratio"], p["check_ori"]) == (s["window"], s["nnratio"], s["check_ori"]) for p in pairs)
        c1, c2 = self.fill(pairs, counts)
        self.grid(s["gp"])
        capi.check(self.search(s["gp"], s["window"], s["nnratio"], s["check_ori"]), self.ctx.handle, "search_for_initialization_device")
        nm, m, prev = self.results()
        out = []
        for b in range(self.B):
            n1 = c1[b]
            assert (m[b, n1:] == -1).all(), (pairs[b]["name"], "rows beyond the count")
            assert prev[b, n1:].tobytes() == self.prev_in[b, n1:].tobytes(), (pairs[b]["name"], "vbPrevMatched beyond the count")
            out.append((int(nm[b]), m[b, :n1].copy(), prev[b, :n1].copy()))
        return out

    def free(self):
        for d in self.bufs.values():
            d.free()


@pytest.mark.parametrize("cap1,cap2", M.CAP_PAIRS)
def test_device_entry_at_the_four_layouts(ctx, cap1, cap2):
    """Every scene through the device entry point with buffers of cap1 / cap2 slots and counts equal to the scene's sizes: the LDS
    layout of k_init_assign follows from the caps alone (staged tables and / or a second list buffer)."""
    assert M.assign_mode(cap1, cap2)[0] == {0: 3, 1: 1, 2: 2, 3: 0}[M.CAP_PAIRS.index((cap1, cap2))]
    call = _DeviceCall(ctx, 1, cap1, cap2)
    try:
        for s in S.all_scenes():
            got = call.run([s])[0]
            want = _expected(s)[0]
            assert _same(got, want), _rows(s, got, want)
    finally:
        call.free()


def _at_window(s, window):
    """The scene under another window (a batch has one window for all its pairs); what it then computes is the model's business."""
    out = dict(s, name="%s@%d" % (s["name"], window), window=window)
    out.pop("_cands", None)
    return out


def test_batched_pairs(ctx):
    """B = 5 in one call, cap1 = 130 != cap2 = 460, the line window for all: the ladder; the 64 features that take one feature
    from each other; a pair with no feature of frame 1; one with no feature of frame 2; and one whose frame 1 fills cap1 (long lists on
    both sides of a round boundary)."""
    ladder = S.by_name("ladder")
    chain = _at_window(S.by_name(S.CHAIN_64), S.LINE_WINDOW)
    long_ = S.by_name("long_between_62_63_64_65")
    full = S.by_name("long_between_126_127_128_129")
    pairs = [ladder, chain, ladder, long_, full]
    counts = [(len(ladder["k1"]), len(ladder["k2"])), (len(chain["k1"]), len(chain["k2"])), (0, len(ladder["k2"])),
              (len(long_["k1"]), 0), (len(full["k1"]), len(full["k2"]))]
    call = _DeviceCall(ctx, 5, 130, 460)
    assert counts[4][0] == call.cap1 and call.cap1 != call.cap2
    try:
        got = call.run(pairs, counts)
    finally:
        call.free()
    for b, (s, (n1, n2)) in enumerate(zip(pairs, counts)):
        if n1 == 0 or n2 == 0:
            assert got[b][0] == 0 and (got[b][1] == -1).all() and got[b][2].tobytes() == s["prev"][:n1].tobytes(), b
            continue
        single = _host(ctx, s)
        assert _same(got[b], single) and _same(got[b], _expected(s)[0]), (b, _rows(s, got[b], _expected(s)[0]))
    assert [g[0] for g in got] == [10, 1, 0, 0, 4]


def test_largest_caps(ctx):
    """(5735, 5734): the match tables take exactly the 112 KB the API allows -- the round-boundary scene runs and agrees.
    (5736, 5734): one slot more is refused before anything is launched, the outputs keep their fill pattern."""
    from orbhip import capi
    s = S.by_name(S.ROUND_BOUNDARY)
    assert M.assign_tables(5735, 5734) == 112 * 1024 and M.assign_mode(5735, 5734)[0] == 0
    call = _DeviceCall(ctx, 1, 5735, 5734)
    try:
        got = call.run([s])[0]
        assert _same(got, _expected(s)[0]), _rows(s, got, _expected(s)[0])
    finally:
        call.free()
    call = _DeviceCall(ctx, 1, 5736, 5734)
    try:
        call.fill([s])
        call.grid(s["gp"])
        rc = call.search(s["gp"], s["window"], s["nnratio"], s["check_ori"])
        assert rc == E_ARG and "cap too large" in capi.last_error(ctx.handle)
        nm, m, prev = call.results()
        assert (nm == 0x5A5A5A5A).all() and (m == 0x5A5A5A5A).all() and prev.tobytes() == call.prev_in.tobytes()
    finally:
        call.free()
    got = _host(ctx, s)                                     # the context is still usable after the error
    assert _same(got, _expected(s)[0])


# ---- ORBHIP_INIT_K: the limits between sorted lists, unsorted lists and the rescan, moved ------------------------------------

def child_main(path_out):
    """Runs in the child process (ORBHIP_INIT_K set: the ablation build reads it once)."""
    from orbhip import capi
    from orbhip.extractor import ORBextractor
    out = dict(lib=np.array(os.path.basename(capi.LIB_PATH)))
    ex = ORBextractor(500, max_w=320, max_h=240)
    for i, s in enumerate(S.all_scenes()):
        out["n%d" % i], out["m%d" % i], out["p%d" % i] = _host(ex, s)
    ex.close()
    np.savez(path_out, **out)


@pytest.mark.parametrize("k", [1, 64])
def test_list_limits_moved(tmp_path, k):
    """ORBHIP_INIT_K = 1: a list of one entry is sorted, everything longer is rescanned.  = 64: lists of up to 64 are sorted,
    everything longer is rescanned (no unsorted lists).  Every scene in one child process, compared with the model here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\nfor p in %r: sys.path.insert(0, p)\nimport test_init_search_edges_gpu as T\nT.child_main(%r)\n"
            % ([os.path.join(root, "tests"), os.path.join(root, "vi-orb-slam-icra2018_amd")], str(tmp_path / "out.npz")))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, ORBHIP_INIT_K=str(k)), timeout=300)
    z = np.load(tmp_path / "out.npz")
    assert str(z["lib"]) == "liborbhip_ablation.so"
    for i, s in enumerate(S.all_scenes()):
        got, want = (int(z["n%d" % i]), z["m%d" % i], z["p%d" % i]), _expected(s)[0]
        assert _same(got, want), _rows(s, got, want)
