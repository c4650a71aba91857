"""Python mirror of the key-frame database (ref: src/KeyFrameDatabase.cc) over the orbhip_kfdb_* C ABI (include/orbhip.h).
BowVectors are the (word ids, values) pairs ORBVocabulary.transform returns; key frames are named by integer keys."""
import ctypes as C

import numpy as np

from . import capi
from .capi import _p, check

RELOC, LOOP = 0, 1


def _bow(bow):
    w, v = bow
    return np.ascontiguousarray(w, np.uint32), np.ascontiguousarray(v, np.float64)


class KeyFrameDatabase:
    def __init__(self, ctx, nwords, max_kfs=65536, delta_max=0):
        """ctx: an ORBextractor (its device context holds the database); nwords: ORBVocabulary.nwords."""
        self._ctx = ctx
        self._L = capi.load()
        self.max_kfs = max_kfs
        check(self._L.orbhip_kfdb_init(ctx.handle, nwords, max_kfs, delta_max), ctx.handle, "orbhip_kfdb_init")

    def _check(self, rc, what):
        check(rc, self._ctx.handle, what)

    def add(self, key, bow):                                   # ref: KeyFrameDatabase.cc:40-46
        w, v = _bow(bow)
        self._check(self._L.orbhip_kfdb_add(self._ctx.handle, int(key), _p(w), _p(v), len(w)), "orbhip_kfdb_add")

    def erase(self, key):                                      # ref :48-68
        self._check(self._L.orbhip_kfdb_erase(self._ctx.handle, int(key)), "orbhip_kfdb_erase")

    def clear(self):                                           # ref :70-74
        self._check(self._L.orbhip_kfdb_clear(self._ctx.handle), "orbhip_kfdb_clear")

    def set_covis(self, key, neighbours):
        """GetBestCovisibilityKeyFrames(10) of `key`, as keys, best first."""
        nb = np.ascontiguousarray(neighbours, np.uint64)
        self._check(self._L.orbhip_kfdb_set_covis(self._ctx.handle, int(key), _p(nb), len(nb)), "orbhip_kfdb_set_covis")

    def info(self):
        """(live, delta, tombstones, rebuilds)."""
        a, b, t = C.c_int(), C.c_int(), C.c_int()
        r = C.c_longlong()
        self._check(self._L.orbhip_kfdb_info(self._ctx.handle, C.byref(a), C.byref(b), C.byref(t), C.byref(r)), "orbhip_kfdb_info")
        return a.value, b.value, t.value, r.value

    def score(self, mode, bow, excluded=()):
        """Phases 1-3 of one query: (keys, counts, scores, min_common) of every key frame sharing a word, reference order."""
        w, v = _bow(bow)
        x = np.ascontiguousarray(excluded, np.uint64)
        cap = self.max_kfs
        keys = np.empty(cap, np.uint64)
        cnt = np.empty(cap, np.int32)
        sc = np.empty(cap, np.float32)
        n, mc = C.c_int(), C.c_int()
        self._check(self._L.orbhip_kfdb_score(self._ctx.handle, mode, _p(w), _p(v), len(w), _p(x) if len(x) else None, len(x),
                                              _p(keys), _p(cnt), _p(sc), cap, C.byref(n), C.byref(mc)), "orbhip_kfdb_score")
        return keys[:n.value].copy(), cnt[:n.value].copy(), sc[:n.value].copy(), mc.value

    @staticmethod
    def _pack(mode, bows, excluded):
        B = len(bows)
        ws, vs = zip(*[_bow(b) for b in bows]) if B else ((), ())
        qoff = np.zeros(B + 1, np.int32)
        qoff[1:] = np.cumsum([len(w) for w in ws])
        qw = np.concatenate(ws).astype(np.uint32) if B and qoff[-1] else np.zeros(1, np.uint32)
        qv = np.concatenate(vs).astype(np.float64) if B and qoff[-1] else np.zeros(1, np.float64)
        ex = [np.asarray(e, np.uint64) for e in (excluded if excluded is not None else [()] * B)]
        xoff = np.zeros(B + 1, np.int32)
        xoff[1:] = np.cumsum([len(e) for e in ex])
        xk = np.concatenate(ex).astype(np.uint64) if xoff[-1] else np.zeros(1, np.uint64)
        return qoff, qw, qv, xoff, xk

    def detect(self, mode, bows, excluded=None, min_score=0.0, cap=None):
        """B queries (a list of BowVectors) as B sequential DetectRelocalizationCandidates / DetectLoopCandidates calls:
        a list of B arrays of candidate keys.  cap: first output capacity (default B * 64); a call that needs more fails
        without changing the database and is repeated with the size it reported."""
        B = len(bows)
        qoff, qw, qv, xoff, xk = self._pack(mode, bows, excluded)
        cap = max(1, B * 64) if cap is None else int(cap)
        while True:
            off = np.zeros(B + 1, np.int32)
            keys = np.empty(max(cap, 1), np.uint64)
            rc = self._L.orbhip_kfdb_detect(self._ctx.handle, mode, B, _p(qoff), _p(qw), _p(qv), _p(xoff), _p(xk),
                                            float(min_score), _p(off), _p(keys), cap)
            if rc == -3 and off[B] > cap:
                cap = int(off[B])
                continue
            self._check(rc, "orbhip_kfdb_detect")
            return [keys[off[b]:off[b + 1]].copy() for b in range(B)]

    def set_timing(self, on=True):
        self._check(self._L.orbhip_kfdb_set_timing(self._ctx.handle, int(bool(on))), "orbhip_kfdb_set_timing")

    def phase_times(self):
        """ms of the last query call: walk, max, score, order, accumulate, retain (orbhip_kfdb_phase_times)"""
        ms = np.zeros(6, np.float32)
        self._check(self._L.orbhip_kfdb_phase_times(self._ctx.handle, _p(ms)), "orbhip_kfdb_phase_times")
        return ms

    def detect_device(self, mode, B, d_qoff, d_qword, d_qvalue, d_xoff, d_xkey, min_score, d_out_off, d_out_keys, out_cap):
        """orbhip_kfdb_detect_device on device pointers (ints): queries / excluded keys as pack() lays them out, candidates
        as CSR.  Synchronises (include/orbhip.h)."""
        vp = lambda x: C.c_void_p(int(x)) if x else None
        self._check(self._L.orbhip_kfdb_detect_device(self._ctx.handle, mode, B, vp(d_qoff), vp(d_qword), vp(d_qvalue),
                                                      vp(d_xoff), vp(d_xkey), float(min_score), vp(d_out_off),
                                                      vp(d_out_keys), int(out_cap)), "orbhip_kfdb_detect_device")

    pack = staticmethod(lambda mode, bows, excluded=None: KeyFrameDatabase._pack(mode, bows, excluded))
