"""orbhip_search_last_frame / orbhip_search_keyframe_points / orbhip_search_last_frame_device on the device against the independent
model (tests/projtrack_model.py) by bit pattern -- queries as 32-byte records, match[], n_active, nmatches -- and against the path
that existed before them: the model's queries and the points' descriptors uploaded to orbhip_search_by_projection, which runs
none of the new kernels.  tests/test_projtrack_model.py shows on the CPU that the scenes contain what these tests rely on."""
import ctypes as C

import numpy as np
import pytest

import projtrack_model as PM
import projtrack_scenes as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_ARG, E_SIZE = -1, -2


def _cam_record(cam, th):
    from orbhip import localmap
    return localmap.camera(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"],
                           cam["scale_factors"], cam["log_scale_factor"], cam["viewing_cos_limit"], th)


class Rig:
    """One context: the scene's current frame (with a grid) and source frame as resident sets, the points in the store and in the
    model's store, the source frame's points as a row of the key-frame table."""

    def __init__(self, sc, last_frame, max_points=2048):
        from orbhip import localmap
        from orbhip.extractor import ORBextractor, ORBmatcher
        self.sc, self.last_frame = sc, last_frame
        self.ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
        self.m = ORBmatcher(0.8, True, ctx=self.ex)
        self.m.put_set(S.CUR, sc["kps"], sc["desc"], None, sc["gp"])
        self.m.put_set(S.SRC, sc["src_kps"], sc["src_desc"])
        self.lm = localmap.LocalMap(self.ex, max_points, 8, 1024)
        idx = S.stored(sc, last_frame)
        self.model = S.model_store(sc, idx)
        self.lm.put(sc["keys"][idx], sc["pos"][idx], sc["normal"][idx], sc["min_dist"][idx], sc["max_dist"][idx], sc["pdesc"][idx],
                    sc["flags"][idx])
        self.row = S.row_keys(sc)
        if not last_frame:
            self.lm.kf_put(S.KFROW, self.row)

    def old_path(self, q, qd, u_right, occupied, check_ori, th_high):
        from orbhip import guided
        sc = self.sc
        return guided.SearchByProjection(self.ex, sc["kps"], sc["desc"], sc["gp"], q, qd, u_right, occupied, False, 0.8, check_ori, th_high)

    def check(self, got, want, u_right, occupied, check_ori, th_high):
        gq, gna, gnm, gm = got
        q, code, qd, na, nm, match = want
        assert gq.tobytes() == q.tobytes(), np.nonzero([a.tobytes() != b.tobytes() for a, b in zip(gq, q)])[0]
        assert gna == na and gnm == nm and np.array_equal(gm, match)
        on, om = self.old_path(q, qd, u_right, occupied, check_ori, th_high)
        assert on == gnm and np.array_equal(om, gm)
        return want

    def last(self, oracle, motion, check_ori=True, mono=False, occupied=True, m=None, src_key=S.SRC, th=None):
        sc = self.sc
        m = len(sc["hold"]) if m is None else m
        th = sc["th"] if th is None else th
        ur = None if mono else sc["u_right"]
        occ = sc["occupied"] if occupied else None
        got = self.lm.search_last_frame(S.CUR, len(sc["kps"]), src_key, sc["hold"][:m], _cam_record(sc["cam"], th), motion, ur, occ,
                                        check_ori, sc["th_high"])
        want = PM.search_last_frame(oracle, self.model, sc["cam"], th, sc["hold"][:m], sc["src_kps"][:m], motion, sc["kps"], sc["desc"],
                                    sc["gp"], ur, occ, check_ori, sc["th_high"])
        return self.check(got, want, ur, occ, check_ori, sc["th_high"])

    def kf(self, oracle, check_ori=True, occupied=True, found=None, row=None, set_key=S.SRC, row_key=S.KFROW, th_high=None):
        sc = self.sc
        row = self.row if row is None else row
        found = sc["found"] if found is None else found
        occ = sc["occupied"] if occupied else None
        th_high = sc["th_high"] if th_high is None else th_high
        got = self.lm.search_keyframe_points(S.CUR, len(sc["kps"]), set_key, row_key, len(row), found, _cam_record(sc["cam"], sc["th"]),
                                             occ, check_ori, th_high)
        want = PM.search_keyframe_points(oracle, self.model, sc["cam"], sc["th"], row, found, sc["src_kps"][:len(row)], sc["kps"],
                                         sc["desc"], sc["gp"], occ, check_ori, th_high)
        return self.check(got, want, None, occ, check_ori, th_high)

    def close(self):
        self.m.close()
        self.ex.close()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_last_frame_bit_for_bit(oracle, name):
    sc = S.make(oracle, name)
    rig = Rig(sc, True)
    for motion in ((PM.SAME,) if name == "mono" else (PM.SAME, PM.FORWARD, PM.BACKWARD)):
        w = rig.last(oracle, motion)
        assert w[4] >= 100 and (w[5] == -2).any()
        rig.last(oracle, motion, check_ori=False)
    rig.last(oracle, PM.SAME, occupied=False)
    rig.last(oracle, PM.SAME, mono=True)             # u_right NULL
    rig.last(oracle, PM.SAME, th=2 * sc["th"])       # the caller's second search, with twice the window
    rig.close()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_keyframe_points_bit_for_bit(oracle, name):
    sc = S.make(oracle, name)
    rig = Rig(sc, False)
    w = rig.kf(oracle)
    assert w[4] >= 100 and (w[5] == -2).any()
    rig.kf(oracle, check_ori=False)
    rig.kf(oracle, occupied=False)
    rig.kf(oracle, found=np.zeros(0, np.uint64))
    rig.kf(oracle, th_high=64)                       # ORBdist of the second relocalisation search
    rig.close()


def test_counts_at_wave_and_block_edges(oracle):
    """1, 63, 64, 65, 255, 256, 257 source features: the ballot count of one wave, of a block, and of the block after it."""
    sc = S.make(oracle, "stereo")
    rig = Rig(sc, True)
    rig.lm.put(sc["keys"][sc["unknown"]], sc["pos"][sc["unknown"]], sc["normal"][sc["unknown"]], sc["min_dist"][sc["unknown"]],
               sc["max_dist"][sc["unknown"]], sc["pdesc"][sc["unknown"]], sc["flags"][sc["unknown"]])     # the rows need every key
    rig.model = S.model_store(sc, np.arange(len(sc["keys"])))
    total = 0
    for k, m in enumerate((1, 63, 64, 65, 255, 256, 257)):
        key = 0x300 + k
        rig.m.put_set(key, sc["src_kps"][:m], sc["src_desc"][:m])
        w = rig.last(oracle, PM.SAME, m=m, src_key=key)
        total += w[3]
        rig.lm.kf_put(0x400 + k, sc["hold"][:m])
        w = rig.kf(oracle, row=sc["hold"][:m], set_key=key, row_key=0x400 + k)
        total += w[3]
    assert total > 700
    rig.close()


def test_edge_scene(oracle):
    sc = S.edge_scene()
    for last_frame in (True, False):
        rig = Rig(sc, last_frame)
        if last_frame:
            for motion in (PM.SAME, PM.FORWARD, PM.BACKWARD):
                for check_ori in (True, False):
                    rig.last(oracle, motion, check_ori)
            rig.last(oracle, PM.SAME, mono=True)
            occ = sc["occupied"].copy()
            occ[sc["ix"]["inside"]] = 1
            sc2 = dict(sc, occupied=occ)
            rig.sc = sc2
            w = rig.last(oracle, PM.SAME)
            assert w[5][sc["ix"]["inside"]] == -1
            rig.sc = sc
        else:
            for check_ori in (True, False):
                rig.kf(oracle, check_ori)
        rig.close()


def test_found_marks_are_cleared_and_stale_entries_resolve_to_nothing(oracle):
    sc = S.make(oracle, "mono")
    rig = Rig(sc, False)
    frame_keys = rig.row[::3]
    before = rig.lm.vote(frame_keys)
    base = rig.kf(oracle)
    rig.kf(oracle, found=np.concatenate([sc["found"], sc["found"][:5], np.array([0, 12345], np.uint64)]))   # repeats, 0, unknown
    after = rig.lm.vote(frame_keys)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[1].sum() > 100
    # points leave the map: the reference's SetBadFlag empties the key frame's entries, the table's entries go stale
    active = np.nonzero(base[1] == PM.ACTIVE)[0]
    gone = active[:40]
    old_slots = rig.lm.slots(rig.row[gone])
    rig.lm.erase(rig.row[gone])
    rig.model.erase(rig.row[gone])
    row = rig.row.copy()
    row[gone] = 0
    w = rig.kf(oracle, row=row)
    assert w[3] == base[3] - 40
    # their slots go to other points: the entries still resolve to nothing
    fresh = (np.arange(40, dtype=np.uint64) + np.uint64(1)) * np.uint64(1000003)
    a = [sc[k][gone] for k in ("pos", "normal", "min_dist", "max_dist", "pdesc", "flags")]
    rig.lm.put(fresh, *a)
    rig.model.put(fresh, *a)
    assert set(rig.lm.slots(fresh)) == set(old_slots)
    w2 = rig.kf(oracle, row=row)
    assert w2[3] == w[3] and np.array_equal(w2[5], w[5])
    # the same points under their new keys in a row of their own
    row3 = row.copy()
    row3[gone] = fresh
    rig.lm.kf_put(S.KFROW, row3)
    w3 = rig.kf(oracle, row=row3)
    assert w3[3] == base[3]
    rig.close()


def test_bad_flag_after_the_fact(oracle):
    """A point turns bad: the last-frame form keeps it (the reference does not test isBad() there), the key-frame form drops it."""
    sc = S.make(oracle, "stereo")
    for last_frame in (True, False):
        rig = Rig(sc, last_frame)
        base = rig.last(oracle, PM.SAME) if last_frame else rig.kf(oracle)
        pick = np.nonzero(base[1] == PM.ACTIVE)[0][:25]
        keys = (sc["hold"] if last_frame else rig.row)[pick]
        fl = np.array([rig.model.pts[int(k)][5] | 2 for k in keys], np.uint8)
        rig.lm.update_flags(keys, fl)
        rig.model.update_flags(keys, fl)
        w = rig.last(oracle, PM.SAME) if last_frame else rig.kf(oracle)
        assert w[3] == (base[3] if last_frame else base[3] - 25)
        rig.close()


def test_device_form_batch_of_three(oracle):
    import hiprt
    from orbhip import capi, localmap
    sc = S.make(oracle, "stereo")
    rig = Rig(sc, True)
    B, n, N = 3, len(sc["kps"]), len(sc["hold"])
    cap, capq = n + 5, N + 3
    counts = (N, 0, 130)                               # unequal, and one frame without points
    motions = (PM.FORWARD, PM.SAME, PM.BACKWARD)
    rng = np.random.default_rng(2)
    cams = np.zeros(B, localmap.CAMERA_DTYPE)
    keys = np.zeros((B, capq), np.uint64)
    lkps = np.zeros((B, capq), capi.KP_DTYPE)
    camd = []
    for b in range(B):
        R, t, Ow = S.LS.pose(rng) if b else (sc["cam"]["Rcw"], sc["cam"]["tcw"], sc["cam"]["Ow"])
        camd.append(dict(sc["cam"], Rcw=R, tcw=t, Ow=Ow))
        cams[b] = _cam_record(camd[b], sc["th"])[0]
        keys[b, :counts[b]] = sc["hold"][:counts[b]]
        lkps[b, :counts[b]] = sc["src_kps"][:counts[b]]
    slots = rig.lm.slots(keys.ravel()).reshape(B, capq)
    kps = np.zeros((B, cap), capi.KP_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    ur = np.full((B, cap), -1, f32)
    occ = np.zeros((B, cap), np.uint8)
    kps[:, :n], desc[:, :n], ur[:, :n], occ[:, :n] = sc["kps"], sc["desc"], sc["u_right"], sc["occupied"]
    D = hiprt.DevBuf
    d = dict(kps=D.from_numpy(kps), desc=D.from_numpy(desc), cnt=D.from_numpy(np.full(B, n, np.int32)), ur=D.from_numpy(ur),
             occ=D.from_numpy(occ), off=D(B * (64 * 48 + 1) * 4), idx=D(B * cap * 4), cam=D.from_numpy(cams), slots=D.from_numpy(slots),
             lkps=D.from_numpy(lkps), mo=D.from_numpy(np.array(motions, np.int32)), nq=D.from_numpy(np.array(counts, np.int32)),
             q=D(B * capq * 32), na=D.from_numpy(np.full(B, 77, np.int32)), m=D(B * cap * 4), nm=D(B * 4))
    gp = sc["gp"]
    L, h = rig.ex._L, rig.ex.handle
    capi.check(L.orbhip_grid_build_device(h, d["kps"].ptr, d["cnt"].ptr, cap, B, gp[0], gp[1], gp[2], gp[3], d["off"].ptr, d["idx"].ptr),
               h, "grid")
    for rep in range(2):      # twice: n_active is set, not accumulated
        rig.lm.search_last_frame_device(d["kps"].ptr, d["desc"].ptr, d["cnt"].ptr, cap, B, d["ur"].ptr, d["occ"].ptr, gp, d["off"].ptr,
                                        d["idx"].ptr, d["cam"].ptr, d["slots"].ptr, d["lkps"].ptr, d["mo"].ptr, d["nq"].ptr, capq, True,
                                        sc["th_high"], d["q"].ptr if rep else 0, d["na"].ptr, d["m"].ptr, d["nm"].ptr)
    rig.ex.sync()
    q = d["q"].to_numpy(localmap.QUERY_DTYPE, (B, capq))
    na, nm, m = d["na"].to_numpy(np.int32, (B,)), d["nm"].to_numpy(np.int32, (B,)), d["m"].to_numpy(np.int32, (B, cap))
    for b in range(B):
        c = counts[b]
        want = PM.search_last_frame(oracle, rig.model, camd[b], sc["th"], sc["hold"][:c], sc["src_kps"][:c], motions[b], sc["kps"],
                                    sc["desc"], sc["gp"], sc["u_right"], sc["occupied"], True, sc["th_high"])
        assert q[b, :c].tobytes() == want[0].tobytes() and na[b] == want[3] and nm[b] == want[4]
        assert np.array_equal(m[b, :n], want[5]) and (m[b, n:] == -1).all()
    assert na[0] > 100 and nm[0] > 50 and na[1] == 0 and nm[1] == 0 and (m[1] == -1).all() and na[2] > 20
    rig.close()
    for x in d.values():
        x.free()


def test_errors_leave_the_outputs_alone(oracle):
    from orbhip import capi, localmap
    from orbhip.capi import _p
    from orbhip.extractor import ORBextractor, ORBmatcher
    sc = S.edge_scene()
    rig = Rig(sc, False)
    L, h = rig.ex._L, rig.ex.handle
    n, N = len(sc["kps"]), len(sc["hold"])
    cam = _cam_record(sc["cam"], sc["th"])
    rig.m.put_set(0x501, sc["kps"], sc["desc"])                          # no grid
    rig.m.put_set(0x502, sc["src_kps"][:N - 1], sc["src_desc"][:N - 1])  # another size
    big = np.zeros(29800, capi.KP_DTYPE)                                 # 4 n + 4 ceil(n / 32) > 120 KB of LDS
    big["x"], big["y"] = 50, 50
    rig.m.put_set(0x503, big, np.zeros((len(big), 32), np.uint8), None, sc["gp"])
    rig.lm.kf_put(0x601, rig.row[:N - 1])

    def cam_with(**kw):
        c = cam.copy()
        for k, v in kw.items():
            c[k] = v
        return c

    def last(cur=S.CUR, src=S.SRC, nl=N, c=cam, motion=0):
        q, m = np.full(N, 0x5A, np.uint8).repeat(32), np.full(max(n, len(big)), 0x5A5A5A5A, np.int32)
        na, nm = C.c_int(-7), C.c_int(-7)
        keys = np.ascontiguousarray(sc["hold"][:nl] if nl <= N else np.zeros(nl, np.uint64))
        rc = L.orbhip_search_last_frame(h, cur, src, _p(keys), nl, _p(c), motion, _p(sc["u_right"]), _p(sc["occupied"]), 1, 100, _p(q),
                                        C.byref(na), _p(m), C.byref(nm))
        assert (q == 0x5A).all() and (m == 0x5A5A5A5A).all() and na.value == -7 and nm.value == -7
        return rc

    def kf(cur=S.CUR, src=S.SRC, row=S.KFROW, c=cam):
        q, m = np.full(N, 0x5A, np.uint8).repeat(32), np.full(max(n, len(big)), 0x5A5A5A5A, np.int32)
        na, nm = C.c_int(-7), C.c_int(-7)
        rc = L.orbhip_search_keyframe_points(h, cur, src, row, _p(sc["found"]), len(sc["found"]), _p(c), _p(sc["occupied"]), 1, 100,
                                             _p(q), C.byref(na), _p(m), C.byref(nm))
        assert (q == 0x5A).all() and (m == 0x5A5A5A5A).all() and na.value == -7 and nm.value == -7
        return rc

    top = np.int32(len(sc["cam"]["scale_factors"]))
    assert last(cur=0x999) == E_ARG and last(src=0x999) == E_ARG and last(cur=0x501) == E_ARG
    assert last(nl=N - 1) == E_ARG and last(nl=N + 1) == E_ARG and last(src=0) == E_ARG and last(nl=0) == E_ARG
    assert last(motion=3) == E_ARG and last(motion=-1) == E_ARG
    assert last(c=cam_with(nlevels=top - 1)) == E_ARG                    # the set has an octave nlevels - 1
    assert last(c=cam_with(nlevels=0)) == E_ARG and last(c=cam_with(nlevels=17)) == E_ARG
    assert last(c=cam_with(th=np.inf)) == E_ARG and last(c=cam_with(th=np.nan)) == E_ARG
    assert last(cur=0x503) == E_SIZE
    assert kf(cur=0x999) == E_ARG and kf(src=0x999) == E_ARG and kf(cur=0x501) == E_ARG and kf(row=0x999) == E_ARG
    assert kf(src=0x502) == E_ARG and kf(row=0x601) == E_ARG             # row and set differ in length, either way
    assert kf(c=cam_with(nlevels=0)) == E_ARG and kf(c=cam_with(nlevels=17)) == E_ARG and kf(c=cam_with(th=np.inf)) == E_ARG
    assert kf(cur=0x503) == E_SIZE
    # nothing was left behind: the calls still give the model's answer
    rig.kf(oracle)
    # no source features: match all -1, counts 0
    # (a set cannot be empty: key 0 stands for the frame without features)
    rig.lm.kf_put(0x602, np.zeros(0, np.uint64))
    q, na, nm, m = rig.lm.search_last_frame(S.CUR, n, 0, np.zeros(0, np.uint64), cam)
    assert na == 0 and nm == 0 and (m == -1).all() and len(m) == n
    q, na, nm, m = rig.lm.search_keyframe_points(S.CUR, n, 0, 0x602, 0, sc["found"], cam)
    assert na == 0 and nm == 0 and (m == -1).all() and len(m) == n
    rig.close()
    # no store; a store without a key-frame table
    ex = ORBextractor(max_w=128, max_h=128, nfeatures=50, nlevels=1)
    mm = ORBmatcher(0.8, True, ctx=ex)
    mm.put_set(S.CUR, sc["kps"], sc["desc"], None, sc["gp"])
    mm.put_set(S.SRC, sc["src_kps"], sc["src_desc"])
    h = ex.handle
    assert last() == E_ARG and kf() == E_ARG
    localmap.LocalMap(ex, 64)
    assert kf() == E_ARG
    mm.close()
    ex.close()
