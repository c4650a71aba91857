"""k_local_frustum on every comparison's edge (tests/localmap_edges.py): per-point records by bit pattern, n_to_match, match[] and
nmatches against the independent model for inputs exactly on each boundary and one float step to each side; the cameras that
differ per case (image bounds, viewing_cos_limit, th, pyramid shape) as rows of the batched device form, whose consecutive rows
alternate (log_scale_factor, nlevels) so that the per-context threshold-table cache is crossed in every direction; the radius
through planted frame features whose window membership flips between 2.5 and 4.0 scale factors; and the launch's own geometry
(capQ around the block size, nq above capQ, empty rows, slots outside the store, sentinels around every output)."""
import ctypes as C

import numpy as np
import pytest

import localmap_edges as edges
import localmap_model as M
from test_localmap_gpu import FRAME, Rig, _cam_record

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 4096                 # sentinel bytes on either side of every output buffer
SENTINEL = 0xA5
_cache = {}


def _scene(oracle):
    if "sc" not in _cache:
        sc = edges.make(oracle)
        tally = edges.verify(oracle, sc)            # (every case hits its target in the model before anything reaches the device)
        print("edge tallies:", {"%s/%s" % k: v for k, v in sorted(tally.items())}, "refused shapes:", sc["refused"] or "none")
        _cache["sc"] = sc
    return _cache["sc"]


def _check_cases(sc, cam_id, pts):
    """The device's record of every case of this camera says what the builder meant."""
    n = 0
    for kind, side, cid, idx, code, lv in sc["cases"]:
        if cid != cam_id:
            continue
        p = pts[idx]
        assert p["in_view"] == (1 if code == M.IN_VIEW else 0), (kind, side, cid, idx)
        if code == M.IN_VIEW and lv is not None:
            assert p["level"] == lv, (kind, side, cid, idx, int(p["level"]), lv)
        n += 1
    return n


class Guarded:
    """A device buffer with sentinel bytes in front, behind and -- until the call writes them -- inside."""

    def __init__(self, nbytes):
        import hiprt
        self.nbytes = nbytes
        self.buf = hiprt.DevBuf.from_numpy(np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8))
        self.ptr = C.c_void_p(self.buf.ptr.value + GUARD)

    def read(self, dtype, shape):
        raw = self.buf.to_numpy(np.uint8, (self.nbytes + 2 * GUARD,))
        assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + self.nbytes:] == SENTINEL).all(), "a write outside the buffer"
        return raw[GUARD:GUARD + self.nbytes].view(dtype).reshape(shape).copy()

    def free(self):
        self.buf.free()


def _device_search(rig, sc, cams, slots, skip, nq, capq, reps=2):
    """orbhip_search_local_points_device over B rows of the scene's frame, `reps` times into the same buffers.
    Returns (points [B, capq], n_to_match [B], nmatches [B], match [B, cap])."""
    import hiprt
    from orbhip import capi, localmap
    from orbhip.capi import check
    B, n = len(cams), len(sc["kps"])
    cap = n + 13
    kps = np.zeros((B, cap), capi.KP_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    occ = np.zeros((B, cap), np.uint8)
    kps[:, :n], desc[:, :n], occ[:, :n] = sc["kps"], sc["desc"], sc["occupied"]
    D = hiprt.DevBuf
    ins = dict(kps=D.from_numpy(kps), desc=D.from_numpy(desc), cnt=D.from_numpy(np.full(B, n, np.int32)), occ=D.from_numpy(occ),
               off=D(B * (64 * 48 + 1) * 4), idx=D(B * cap * 4), cam=D.from_numpy(cams),
               slots=D.from_numpy(np.ascontiguousarray(slots, np.int32)), skip=D.from_numpy(np.ascontiguousarray(skip, np.uint8)),
               nq=D.from_numpy(np.ascontiguousarray(nq, np.int32)))
    out = dict(pts=Guarded(B * capq * 24), ntm=Guarded(B * 4), m=Guarded(B * cap * 4), nm=Guarded(B * 4))
    gp = sc["gp"]
    L, h = rig.ex._L, rig.ex.handle
    check(L.orbhip_grid_build_device(h, ins["kps"].ptr, ins["cnt"].ptr, cap, B, gp[0], gp[1], gp[2], gp[3], ins["off"].ptr,
                                     ins["idx"].ptr), h, "grid")
    for rep in range(reps):     # more than once: n_to_match is set, not accumulated
        check(L.orbhip_search_local_points_device(h, ins["kps"].ptr, ins["desc"].ptr, ins["cnt"].ptr, cap, B, None, ins["occ"].ptr, gp[0],
                                                  gp[1], gp[2], gp[3], ins["off"].ptr, ins["idx"].ptr, ins["cam"].ptr, ins["slots"].ptr,
                                                  ins["skip"].ptr, ins["nq"].ptr, capq, 0.8, out["pts"].ptr, out["ntm"].ptr, out["m"].ptr,
                                                  out["nm"].ptr), h, "orbhip_search_local_points_device")
    rig.ex.sync()
    res = (out["pts"].read(localmap.POINT_DTYPE, (B, capq)), out["ntm"].read(np.int32, (B,)), out["nm"].read(np.int32, (B,)),
           out["m"].read(np.int32, (B, cap)))
    for x in list(ins.values()) + list(out.values()):
        x.free()
    return res


def _untouched(pts_row):
    return (pts_row.view(np.uint8) == SENTINEL).all()


@pytest.mark.parametrize("cam_id", ["base", "pcz_sum", "pcz_raw", "pcz_neg"])
def test_shared_camera_edges_in_the_single_call(oracle, cam_id):
    """Near, far, the level thresholds of (1.2, 8) and view_cos around (float)0.998 under the scene's camera; PcZ of +0.0f, -0.0f
    and the smallest normals under three cameras built for it (u, v of +-inf or NaN: the model's comparisons decide, and the
    record is compared by bit pattern like any other)."""
    sc = _scene(oracle)
    cam, th, shape = sc["cams"][cam_id]
    rig = Rig(dict(sc, cam=cam))
    none = np.zeros(len(sc["keys"]), np.uint8)
    for t in ((1.0, 3.0) if cam_id == "base" else (1.0,)):
        rec, code, ntm, nm, match = rig.compare(oracle, sc["keys"], none, t, check_old_path=True)
        # (compare: the device's records are rec; the floor on the PcZ cases is over the three cameras, in edges.verify)
        assert _check_cases(sc, cam_id, rec) == sum(c[2] == cam_id for c in sc["cases"]) > 0 and ntm > 0
        if cam_id == "base" and t == 1.0:
            assert nm >= 100
            for j, f in sc["planted"].items():      # the planted feature is matched exactly when the radius is 4.0 scale factors
                assert (match[f] == j) == (not np.float64(rec["view_cos"][j]) > 0.998)
    rig.close()


@pytest.mark.parametrize("part", [0, 1, 2])
def test_own_camera_rows_in_the_batched_form(oracle, part):
    """Image bounds, viewing_cos_limit, th and the pyramid shape are camera parameters: one camera per row, consecutive rows with
    a different (log_scale_factor, nlevels)."""
    from orbhip import guided, localmap
    sc = _scene(oracle)
    model = edges.model_all(oracle, sc)
    per = -(-len(sc["rows"]) // 3)
    rows = sc["rows"][part * per:(part + 1) * per]
    assert 0 < len(rows) <= 32
    shapes = [sc["cams"][r][2] for r in rows]
    assert all(a != b for a, b in zip(shapes, shapes[1:]))
    pairs = list(zip(shapes, shapes[1:]))
    assert any(a[1] == b[1] and a[0] != b[0] for a, b in pairs) and any(a[0] == b[0] and a[1] != b[1] for a, b in pairs)
    assert any(shapes.index(s) < i - 1 for i, s in enumerate(shapes))      # a shape comes back after others used the cache
    rig = Rig(sc)
    cams = np.concatenate([_cam_record(sc["cams"][r][0], sc["cams"][r][1]) for r in rows])
    prepared = rig.lm.prepare(cams)
    for b, shape in enumerate(shapes):
        T = localmap.predict_scale_table(edges.shape_params(shape)[1], shape[1])
        got = prepared["level_ratio"][b]
        assert np.array_equal(got[:shape[1] - 1].view(np.uint32), T.view(np.uint32)), (b, shape)
        assert (got[shape[1] - 1:].view(np.uint32) == 0).all() and prepared["reserved"][b] == 0, (b, shape)
    B, nq = len(rows), len(sc["keys"])
    capq = nq + 5
    slots = np.full((B, capq), -1, np.int32)
    slots[:, :nq] = rig.lm.slots(sc["keys"])
    pts, ntm, nm, m = _device_search(rig, sc, prepared, slots, np.zeros((B, capq), np.uint8), np.full(B, nq, np.int32), capq)
    n = len(sc["kps"])
    none = np.zeros(nq, np.uint8)
    ncases = 0
    for b, r in enumerate(rows):
        rec, code, wntm, wnm, wmatch, q, qd = model[r]
        for f in ("u", "v", "proj_xr", "view_cos"):
            assert np.array_equal(pts[b, :nq][f].view(np.uint32), rec[f].view(np.uint32)), (r, f)
        assert np.array_equal(pts[b, :nq]["level"], rec["level"]) and np.array_equal(pts[b, :nq]["in_view"], rec["in_view"]), r
        assert _untouched(pts[b, nq:])
        assert ntm[b] == wntm and nm[b] == wnm and np.array_equal(m[b, :n], wmatch) and (m[b, n:] == -1).all(), r
        assert wntm > 0 and wnm > 0
        ncases += _check_cases(sc, r, pts[b])
        # old path = new path: the window search fed with the model's queries (the radius is in them, not in the record)
        on, om = guided.SearchByProjection(rig.ex, sc["kps"], sc["desc"], sc["gp"], q, qd, None, sc["occupied"], True, 0.8, False, 100)
        assert on == nm[b] and np.array_equal(om, m[b, :n]), r
        if sc["cams"][r][2] == edges.BASE_SHAPE and r >= sc["first_plain"]:     # the th rows: every planted feature decides
            for j, f in sc["planted"].items():
                assert (m[b, f] == j) == (not np.float64(rec["view_cos"][j]) > 0.998), (r, j)
        if b < 6:               # the single call prepares its own camera: the cache is crossed there as well
            one = rig.lm.search(FRAME, n, cams[b:b + 1], sc["keys"], none, 0.8, None, sc["occupied"])
            assert pts[b, :nq].tobytes() == one[0].tobytes() and one[1] == ntm[b] and one[2] == nm[b] and np.array_equal(one[3], m[b, :n])
    assert ncases >= 5 * sum(r < sc["first_plain"] for r in rows)
    rig.close()


def _model_rows(oracle, rig, sc, keys, skip, nq):
    cam, th, _ = sc["cams"]["base"]
    return [M.search_local_points(oracle, rig.model, cam, th, keys[b, :nq[b]], skip[b, :nq[b]], sc["kps"], sc["desc"], sc["gp"], 0.8, None,
                                  sc["occupied"]) for b in range(len(nq))]


def _compare_rows(sc, want, got, nq_eff, capq):
    pts, ntm, nm, m = got
    n = len(sc["kps"])
    for b, (rec, code, wntm, wnm, wmatch, q, qd) in enumerate(want):
        k = nq_eff[b]
        for f in ("u", "v", "proj_xr", "view_cos", "level", "in_view"):
            assert np.array_equal(pts[b, :k][f].view(np.uint32), rec[f].view(np.uint32)), (b, f)
        assert _untouched(pts[b, k:]), b             # rows past nq (or past capQ) are never written
        assert ntm[b] == wntm and nm[b] == wnm, (b, ntm[b], wntm, nm[b], wnm)
        assert np.array_equal(m[b, :n], wmatch if len(wmatch) else np.full(n, -1, np.int32)) and (m[b, n:] == -1).all(), b


@pytest.mark.parametrize("capq", [255, 256, 257, 513])
def test_capq_around_the_block_size(oracle, capq):
    """nq = capQ at one lane below, at and above one block of 256 lanes, and one above two blocks."""
    sc = _scene(oracle)
    rig = Rig(sc)
    rng = np.random.default_rng(capq)
    B = 3
    keys = np.stack([rng.permutation(sc["keys"])[:capq] for b in range(B)])
    skip = (rng.random((B, capq)) < 0.05).astype(np.uint8)
    nq = np.full(B, capq, np.int32)
    cam, th, _ = sc["cams"]["base"]
    cams = rig.lm.prepare(np.concatenate([_cam_record(cam, th)] * B))
    got = _device_search(rig, sc, cams, rig.lm.slots(keys.ravel()).reshape(B, capq), skip, nq, capq)
    want = _model_rows(oracle, rig, sc, keys, skip, nq)
    _compare_rows(sc, want, got, nq, capq)
    assert all(w[2] > 0 and w[3] > 0 for w in want)
    rig.close()


def test_nq_above_capq_empty_rows_and_slots_outside_the_store(oracle):
    """nq[b] > capQ is clamped (in the middle of the batch and in its last row, where a write past capQ would land in the
    sentinel); nq[b] = 0 between two full rows; slots of -1 and of max_points are not in view and never read."""
    sc = _scene(oracle)
    max_points = len(sc["keys"]) + 3
    rig = Rig(sc, max_points=max_points)
    rng = np.random.default_rng(77)
    B, capq = 6, 300
    nq = np.array([capq, capq + 1, 0, capq - 1, 257, capq + 1000], np.int32)
    nq_eff = np.minimum(nq, capq)
    keys = np.stack([rng.permutation(sc["keys"])[:capq] for b in range(B)])
    skip = (rng.random((B, capq)) < 0.05).astype(np.uint8)
    slots = rig.lm.slots(keys.ravel()).reshape(B, capq)
    assert (slots >= 0).all() and slots.max() < max_points
    unknown = np.uint64(3)                                   # (a key the model's store does not hold: not tested)
    for b in range(B):
        at = rng.choice(max(int(nq_eff[b]), 24), 24, replace=False)
        slots[b, at[:12]], slots[b, at[12:]] = -1, max_points
        keys[b, at] = unknown
    slots[0, capq - 1], keys[0, capq - 1] = max_points, unknown       # the last lane of a row
    slots[3, 0], keys[3, 0] = -1, unknown
    cam, th, _ = sc["cams"]["base"]
    cams = rig.lm.prepare(np.concatenate([_cam_record(cam, th)] * B))
    got = _device_search(rig, sc, cams, slots, skip, nq, capq, reps=3)
    want = _model_rows(oracle, rig, sc, keys, skip, nq_eff)
    _compare_rows(sc, want, got, nq_eff, capq)
    assert got[1][2] == 0 and got[2][2] == 0 and (got[3][2] == -1).all()          # the empty row
    assert all(w[2] > 0 and w[3] > 0 for b, w in enumerate(want) if nq[b] > 0)
    for b in range(B):
        gone = np.nonzero(keys[b, :nq_eff[b]] == unknown)[0]
        assert len(gone) >= (24 if nq_eff[b] else 0) and (got[0][b, gone].view(np.uint8) == 0).all() and (want[b][1][gone] == M.NOT_TESTED).all()
    rig.close()
