"""The RGB-D sensor path on the device against the independent model (tests/rgbd_model.py) and the CPU oracle: grey conversion
byte for byte in every format, width class, stride and alignment; colour extraction equal to grey extraction of the model's
image; orbhip_frame_build_rgbd equal to orbhip_frame_build plus the model's depth, by float bit patterns, with the TUM1 camera;
the batched device forms; the resident chain; the error paths."""
import ctypes as C

import numpy as np
import pytest

import rgbd_model as M
import rgbd_scenes as scenes

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = (M.FMT_RGB, M.FMT_BGR, M.FMT_RGBA, M.FMT_BGRA)
WIDTHS, HEIGHTS = (640, 641, 642, 643, 37, 5, 1), (480, 19, 1)
POISON = 0xA5


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _align(v, a):
    return (v + a - 1) // a * a


def _strided(rng, h, w, ch, stride, offset):
    """A random (h, w, ch) image inside a byte buffer: rows `stride` apart, the first pixel `offset` bytes behind an aligned base."""
    buf = np.zeros(stride * h + offset + 64, np.uint8)
    base = (-buf.ctypes.data) % 64
    buf[:] = rng.integers(0, 256, buf.size, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[base + offset:], (h, w, ch), (stride, ch, 1))
    assert (view.ctypes.data - offset) % 64 == 0
    return buf, view


@pytest.fixture(scope="module")
def ex():
    from orbhip.extractor import ORBextractor
    e = ORBextractor(1000, max_w=640, max_h=600, max_batch=8)
    yield e
    e.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_grey_host_form(ex, fmt):
    """The host form stages rows packed, so on the device row y of a 3-channel image starts at y * w * 3 mod 4: every alignment
    for w % 4 != 0 -- the kernel's byte-by-byte rows.  `offset` varies the HOST pointer only (the copy-in absorbs it)."""
    from orbhip import rgbd
    rng = np.random.default_rng(100 + fmt)
    ch = M.CHANNELS[fmt]
    for w in WIDTHS:
        for h in HEIGHTS:
            for stride in (w * ch, w * ch + 5):
                for offset in range(4):
                    keep, img = _strided(rng, h, w, ch, stride, offset)
                    for dstride in (_align(w, 64), _align(w, 4), w + 3):
                        out = np.full((h, dstride), POISON, np.uint8)
                        rgbd.grey(ex, img, fmt, out)
                        want = np.full((h, dstride), POISON, np.uint8)
                        want[:, :w] = M.grey(img, fmt)
                        assert np.array_equal(out, want), (w, h, stride, offset, dstride)


@pytest.mark.parametrize("fmt", FORMATS)
def test_grey_device_form(ex, fmt):
    import hiprt
    from orbhip import rgbd
    rng = np.random.default_rng(200 + fmt)
    ch = M.CHANNELS[fmt]
    for w in WIDTHS:
        for h in HEIGHTS:
            for B in (1, 3, 8):
                for stride in (_align(w * ch, 4), _align(w * ch, 4) + 8):
                    for dstride in (_align(w, 64), _align(w, 4)):
                        sframe, dframe = stride * h + 16, dstride * h + 32
                        src = rng.integers(0, 256, (B, sframe), dtype=np.uint8)
                        d_src, d_dst = hiprt.DevBuf.from_numpy(src), hiprt.DevBuf.from_numpy(np.full((B, dframe), POISON, np.uint8))
                        rgbd.grey_device(ex, d_src.ptr, B, w, h, stride, sframe, fmt, d_dst.ptr, dstride, dframe)
                        ex.sync()
                        got = d_dst.to_numpy(np.uint8, (B, dframe))
                        want = np.full((B, dframe), POISON, np.uint8)
                        for b in range(B):
                            img = np.lib.stride_tricks.as_strided(src[b], (h, w, ch), (stride, ch, 1))
                            np.lib.stride_tricks.as_strided(want[b], (h, w), (dstride, 1))[:] = M.grey(img, fmt)
                        d_src.free()
                        d_dst.free()
                        assert np.array_equal(got, want), (w, h, B, stride, dstride)


def _colour_frames():
    from orbhip import synth
    out = dict(scenes.colourings(scenes.grey_frame()))
    for i, p in enumerate(synth.load_photographs_rgb()):
        out["photograph%d" % i] = p
    return out


def test_extract_color_equals_grey_extraction_and_the_oracle(ex, oracle):
    from orbhip import rgbd
    ref = oracle.Extractor(1000)
    frames = _colour_frames()
    print("colour frames:", {k: v.shape for k, v in frames.items()})
    for name, rgb in frames.items():
        g = M.grey(rgb, M.FMT_RGB)
        k, d = rgbd.extract_color(ex, rgb, M.FMT_RGB)
        gk, gd = ex(g)
        rk, rd = ref(g)
        assert len(k) > 100, name
        assert k.tobytes() == gk.tobytes() and np.array_equal(d, gd), name + ": differs from orbhip_extract on the grey image"
        assert k.tobytes() == rk.tobytes() and np.array_equal(d, rd), name + ": differs from the oracle"
        # four channels, blue first, padded rows
        bgra = np.zeros((rgb.shape[0], rgb.shape[1] + 3, 4), np.uint8)
        bgra[:, :rgb.shape[1], :3], bgra[:, :, 3] = rgb[:, :, ::-1], 99
        k4, d4 = rgbd.extract_color(ex, bgra[:, :rgb.shape[1]], M.FMT_BGRA)
        assert k4.tobytes() == rk.tobytes() and np.array_equal(d4, rd), name
        # ORBHIP_FMT_GREY is orbhip_extract
        k1, d1 = rgbd.extract_color(ex, g, M.FMT_GREY)
        assert k1.tobytes() == rk.tobytes() and np.array_equal(d1, rd), name
        if name != "replicated":
            # the flag is live: the same bytes read as BGR give another image and other features
            kb, db = rgbd.extract_color(ex, rgb, M.FMT_BGR)
            assert not np.array_equal(M.grey(rgb, M.FMT_BGR), g)
            assert kb.tobytes() != k.tobytes() or not np.array_equal(db, d), name
            bk, bd = ref(M.grey(rgb, M.FMT_BGR))
            assert kb.tobytes() == bk.tobytes() and np.array_equal(db, bd), name
    # the host pyramid's level 0 is the grey image
    rgb = frames["tinted"]
    ex.set_host_pyramid(True)
    try:
        rgbd.extract_color(ex, rgb, M.FMT_RGB)
        assert np.array_equal(ex.host_pyramid(0), M.grey(rgb, M.FMT_RGB))
        assert np.array_equal(ex.host_pyramid(1), ex.image_pyramid(1))
    finally:
        ex.set_host_pyramid(False)


def _tum_grid(oracle):
    corners = np.array([[0, 0], [scenes.W, 0], [0, scenes.H], [scenes.W, scenes.H]], f32)
    un = oracle.undistort_points(corners, scenes.K_TUM1, scenes.D_TUM1, scenes.K_TUM1)
    return oracle.grid_params(min(un[0, 0], un[2, 0]), max(un[1, 0], un[3, 0]), min(un[0, 1], un[1, 1]), max(un[2, 1], un[3, 1]))


def test_frame_build_rgbd_tum1(oracle):
    import localmap_scenes
    from orbhip import distributed as Dist, localmap, rgbd
    from orbhip.extractor import ORBextractor, ORBmatcher
    from orbhip.vocabulary import ORBVocabulary
    W, H = scenes.W, scenes.H
    e = ORBextractor(1000, max_w=W, max_h=H)
    voc = ORBVocabulary(e)
    voc.loadFromBinaryBlob(Dist.make_synthetic_vocabulary(52, k=10, L=5))
    gp = _tum_grid(oracle)
    rgb = scenes.colourings(scenes.grey_frame())["tinted"]
    g = M.grey(rgb, M.FMT_RGB)
    depth = scenes.depth_map()
    assert 0.15 < (depth == 0).mean() < 0.25 and depth[depth > 0].min() >= 2500 and depth.max() <= 40000
    K, D = scenes.K_TUM1, scenes.D_TUM1
    m = ORBmatcher(0.8, False)

    def search(res, u_right):
        """the frame the extractor built last as a resident set, then one orbhip_search_local_points"""
        fv = oracle.feature_vector(res["node_id"], res["weight"])
        m.put_set_from_frame(9, e, fv)
        lm = localmap.LocalMap(m._ctx, 4096)
        rng = np.random.default_rng(3)
        sf = (f32(1.2) ** np.arange(8)).astype(f32)
        R, t, Ow = localmap_scenes.pose(rng)
        cam = dict(Rcw=R, tcw=t, Ow=Ow, fx=f32(scenes.FX), fy=f32(scenes.FY), cx=f32(scenes.CX), cy=f32(scenes.CY), mbf=scenes.BF,
                   bounds=(f32(0), f32(W), f32(0), f32(H)), scale_factors=sf, log_scale_factor=f32(np.log(f32(1.2))),
                   viewing_cos_limit=f32(0.5))
        p = localmap_scenes.map_points(rng, cam, res["kps_un"], res["desc"], 2000, W, H)
        lm.put(p["keys"], p["pos"], p["normal"], p["min_dist"], p["max_dist"], p["pdesc"], p["flags"])
        rec = localmap.camera(R, t, Ow, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], cam["bounds"], sf, cam["log_scale_factor"],
                              cam["viewing_cos_limit"], 1.0)
        out = lm.search(9, len(res["kps"]), rec, p["keys"], np.zeros(2000, np.uint8), 0.8, u_right)
        lm.clear()
        return out

    for rnd in range(3):                                    # capture, replay, replay
        got = rgbd.frame_build_rgbd(e, rgb, M.FMT_RGB, depth, scenes.DEPTH_FACTOR, scenes.BF, K, D, gp, 4)
        fp_colour = e.frame_fingerprint()
        s_colour = search(got, got["u_right"]) if rnd == 2 else None
        want = e.frame_build(g, K, D, gp, 4)
        assert fp_colour == e.frame_fingerprint() != 0
        for f in ("kps", "kps_un", "desc", "cell_off", "cell_idx", "word_id", "weight", "node_id"):
            assert got[f].tobytes() == want[f].tobytes(), f
        n = len(got["kps"])
        assert n > 900
        mur, mdz = M.depth_at_keypoints(got["kps"], got["kps_un"], depth, scenes.DEPTH_FACTOR, scenes.BF)
        print("round %d: %d keypoints, %d with a depth, %d without" % (rnd, n, (mdz > 0).sum(), (mdz < 0).sum()))
        assert (mdz > 0).sum() >= 50 and (mdz < 0).sum() >= 50
        assert (got["kps"]["x"].astype(np.int32) != got["kps_un"]["x"].astype(np.int32)).any()
        assert np.array_equal(_bits(got["depth"]), _bits(mdz)) and np.array_equal(_bits(got["u_right"]), _bits(mur))
        # with the wrong keypoint the lookup gives something else: the check above can fail
        wur, wdz = M.depth_at_keypoints(got["kps_un"], got["kps_un"], depth, scenes.DEPTH_FACTOR, scenes.BF)
        assert not np.array_equal(_bits(wdz), _bits(mdz))
    # the frame as a resident set and one SearchLocalPoints with the returned u_right: the same after the grey build
    s_grey = search(want, got["u_right"])
    assert s_colour[1] == s_grey[1] and s_colour[2] == s_grey[2] > 50
    assert s_colour[0].tobytes() == s_grey[0].tobytes() and np.array_equal(s_colour[3], s_grey[3])
    # the oracle's four calls on the model's grey image
    rk, rd = oracle.Extractor(1000)(g)
    assert got["kps"].tobytes() == rk.tobytes() and np.array_equal(got["desc"], rd)
    # a float map that was converted beforehand, no depth at all, a grey frame with a depth map
    conv = (depth.astype(f32) * scenes.DEPTH_FACTOR).astype(f32)
    g2 = rgbd.frame_build_rgbd(e, rgb, M.FMT_RGB, conv, 1.0, scenes.BF, K, D, gp, 4)
    assert np.array_equal(_bits(g2["depth"]), _bits(got["depth"])) and np.array_equal(_bits(g2["u_right"]), _bits(got["u_right"]))
    g3 = rgbd.frame_build_rgbd(e, rgb, M.FMT_RGB, None, 1.0, scenes.BF, K, D, gp, 4)
    assert (g3["depth"] == -1).all() and (g3["u_right"] == -1).all() and g3["kps"].tobytes() == got["kps"].tobytes()
    g4 = rgbd.frame_build_rgbd(e, g, M.FMT_GREY, depth, scenes.DEPTH_FACTOR, scenes.BF, K, D, gp, 4)
    assert g4["kps_un"].tobytes() == got["kps_un"].tobytes() and np.array_equal(_bits(g4["depth"]), _bits(got["depth"]))
    # level 0 of the host pyramid is the grey image
    e.set_host_pyramid(True)
    rgbd.frame_build_rgbd(e, rgb, M.FMT_RGB, depth, scenes.DEPTH_FACTOR, scenes.BF, K, D, gp, 4)
    assert np.array_equal(e.host_pyramid(0), g) and np.array_equal(e.host_pyramid(2), e.image_pyramid(2))
    m.close()
    e.close()


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_rgbd_depth_device(ex, dtype):
    import hiprt
    from orbhip import capi, rgbd
    B, cap, w, h = 8, 700, 200, 120
    rng = np.random.default_rng(31)
    counts = np.array([700, 0, 1, 513, 64, 699, 257, 300], np.int32)
    stride = w * np.dtype(dtype).itemsize + 16
    dframe = stride * h + 8
    raw = np.zeros((B, dframe), np.uint8)
    maps = []
    for b in range(B):
        if dtype == np.uint16:
            d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
            d[rng.random((h, w)) < 0.2] = 0
        else:
            d = (rng.random((h, w)) * 9 - 1).astype(f32)
            d[rng.random((h, w)) < 0.05] = np.nan
        maps.append(d)
        np.lib.stride_tricks.as_strided(raw[b].view(dtype), (h, w), (stride, d.itemsize))[:] = d
    kps, kun = np.zeros((B, cap), capi.KP_DTYPE), np.zeros((B, cap), capi.KP_DTYPE)
    kps["x"], kps["y"] = rng.random((B, cap)) * w, rng.random((B, cap)) * h
    kun["x"] = kps["x"] + rng.standard_normal((B, cap)) * 2
    kps["x"][0, 5], kps["y"][0, 5] = w, 3          # planted at x = w: outside, harmless, no depth
    kps["x"][3, 0], kps["y"][3, 0] = 3, h
    d_kps, d_kun, d_cnt = hiprt.DevBuf.from_numpy(kps), hiprt.DevBuf.from_numpy(kun), hiprt.DevBuf.from_numpy(counts)
    d_map = hiprt.DevBuf.from_numpy(raw)
    dt = rgbd.DEPTH_U16 if dtype == np.uint16 else rgbd.DEPTH_F32
    for factor in (f32(1.0) / f32(5000.0), f32(1.0), f32(1.0) + f32(5e-6), f32(0.5)):
        poison = np.full((B, cap), 123.5, f32)
        d_ur, d_dz = hiprt.DevBuf.from_numpy(poison), hiprt.DevBuf.from_numpy(poison)
        rgbd.rgbd_depth_device(ex, d_kps.ptr, d_kun.ptr, d_cnt.ptr, cap, B, d_map.ptr, dt, w, h, stride, dframe, factor, 40.0, d_ur.ptr,
                               d_dz.ptr)
        ex.sync()
        ur, dz = d_ur.to_numpy(f32, (B, cap)), d_dz.to_numpy(f32, (B, cap))
        for b in range(B):
            n = counts[b]
            mur, mdz = M.depth_at_keypoints(kps[b, :n], kun[b, :n], maps[b], factor, 40.0)
            assert np.array_equal(_bits(dz[b, :n]), _bits(mdz)) and np.array_equal(_bits(ur[b, :n]), _bits(mur)), (b, float(factor))
            assert (dz[b, n:] == 123.5).all() and (ur[b, n:] == 123.5).all(), b
        assert dz[0, 5] == -1 and ur[0, 5] == -1 and dz[3, 0] == -1
        assert (dz[0] > 0).sum() > 100 and (dz[0] == -1).sum() > 20
        d_ur.free()
        d_dz.free()
    # no counts: cap keypoints per frame
    d_ur, d_dz = hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * cap * 4)
    rgbd.rgbd_depth_device(ex, d_kps.ptr, d_kun.ptr, None, cap, B, d_map.ptr, dt, w, h, stride, dframe, 0.5, 40.0, d_ur.ptr, d_dz.ptr)
    ex.sync()
    dz = d_dz.to_numpy(f32, (B, cap))
    mur, mdz = M.depth_at_keypoints(kps[1], kun[1], maps[1], 0.5, 40.0)
    assert np.array_equal(_bits(dz[1]), _bits(mdz))
    for d in (d_kps, d_kun, d_cnt, d_map, d_ur, d_dz):
        d.free()


def test_resident_chain_grey_then_extract(ex, oracle):
    """orbhip_grey_device -> orbhip_extract_batch_device -> orbhip_undistort_keypoints_device -> orbhip_rgbd_depth_device on 8 colour
    frames: the features of 8 single grey extractions, the depths of the model."""
    import hiprt
    from orbhip import capi, rgbd, synth
    from orbhip.capi import check
    B, W, H = 8, scenes.W, scenes.H
    greys = synth.make_frames(71, W, H, B)
    rgb = np.stack([scenes.colourings(greys[b], seed=20 + b)["tinted"] for b in range(B)])
    depth = np.stack([scenes.depth_map(seed=40 + b) for b in range(B)])
    cap = ex.cap
    d_rgb, d_grey, d_depth = hiprt.DevBuf.from_numpy(rgb), hiprt.DevBuf(B * W * H), hiprt.DevBuf.from_numpy(depth)
    d_kps, d_kun, d_desc, d_cnt = hiprt.DevBuf(B * cap * 28), hiprt.DevBuf(B * cap * 28), hiprt.DevBuf(B * cap * 32), hiprt.DevBuf(B * 4)
    d_ur, d_dz = hiprt.DevBuf(B * cap * 4), hiprt.DevBuf(B * cap * 4)
    rgbd.grey_device(ex, d_rgb.ptr, B, W, H, W * 3, W * H * 3, M.FMT_RGB, d_grey.ptr, W, W * H)
    ex.extract_batch_device(d_grey.ptr, B, W, H, W, W * H, d_kps.ptr, d_desc.ptr, cap, d_cnt.ptr)
    K, D = np.ascontiguousarray(scenes.K_TUM1), np.ascontiguousarray(scenes.D_TUM1)
    check(ex._L.orbhip_undistort_keypoints_device(ex.handle, d_kps.ptr, d_cnt.ptr, cap, B, K.ctypes.data, D.ctypes.data, 5, K.ctypes.data,
                                                  d_kun.ptr), ex.handle, "orbhip_undistort_keypoints_device")
    rgbd.rgbd_depth_device(ex, d_kps.ptr, d_kun.ptr, d_cnt.ptr, cap, B, d_depth.ptr, rgbd.DEPTH_U16, W, H, W * 2, W * H * 2,
                           scenes.DEPTH_FACTOR, scenes.BF, d_ur.ptr, d_dz.ptr)
    ex.sync()
    cnt = d_cnt.to_numpy(np.int32, (B,))
    kps, kun = d_kps.to_numpy(capi.KP_DTYPE, (B, cap)), d_kun.to_numpy(capi.KP_DTYPE, (B, cap))
    desc = d_desc.to_numpy(np.uint8, (B, cap, 32))
    ur, dz = d_ur.to_numpy(f32, (B, cap)), d_dz.to_numpy(f32, (B, cap))
    assert np.array_equal(d_grey.to_numpy(np.uint8, (B, H, W)), np.stack([M.grey(rgb[b], M.FMT_RGB) for b in range(B)]))
    ref = oracle.Extractor(1000)
    for b in range(B):
        g = M.grey(rgb[b], M.FMT_RGB)
        k1, d1 = ex(g)
        n = cnt[b]
        assert n == len(k1) > 100 and kps[b, :n].tobytes() == k1.tobytes() and np.array_equal(desc[b, :n], d1), b
        if b < 2:
            rk, rd = ref(g)
            assert k1.tobytes() == rk.tobytes() and np.array_equal(d1, rd)
        mur, mdz = M.depth_at_keypoints(kps[b, :n], kun[b, :n], depth[b], scenes.DEPTH_FACTOR, scenes.BF)
        assert np.array_equal(_bits(dz[b, :n]), _bits(mdz)) and np.array_equal(_bits(ur[b, :n]), _bits(mur)), b
        assert (kps[b, :n]["x"] != kun[b, :n]["x"]).any() and (mdz > 0).sum() >= 50 and (mdz < 0).sum() >= 50
    for d in (d_rgb, d_grey, d_depth, d_kps, d_kun, d_desc, d_cnt, d_ur, d_dz):
        d.free()


def test_error_paths_leave_outputs_and_context_usable(ex, oracle):
    import hiprt
    from orbhip import capi, rgbd
    L = capi.load()
    E_ARG = -1
    rgb = scenes.colourings(scenes.grey_frame())["tinted"]
    W, H = scenes.W, scenes.H
    cap = ex.cap
    kps, kun, desc = np.zeros(cap, capi.KP_DTYPE), np.zeros(cap, capi.KP_DTYPE), np.full((cap, 32), POISON, np.uint8)
    ur, dz = np.full(cap, 7, f32), np.full(cap, 7, f32)
    n = C.c_int(-5)
    out = np.full((H, W), POISON, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def bad(rc):
        assert rc == E_ARG and capi.last_error(ex.handle)

    # orbhip_grey / orbhip_extract_color: unknown format, grey where a colour is asked for, stride below w * channels
    for fmt in (-1, 5, 99):
        bad(L.orbhip_grey(ex.handle, p(rgb), W, H, W * 3, fmt, p(out), W))
        bad(L.orbhip_extract_color(ex.handle, p(rgb), W, H, W * 3, fmt, p(kps), p(desc), cap, C.byref(n), None))
    bad(L.orbhip_grey(ex.handle, p(rgb), W, H, W * 3, M.FMT_GREY, p(out), W))
    bad(L.orbhip_grey(ex.handle, p(rgb), W, H, W * 3 - 1, M.FMT_RGB, p(out), W))
    bad(L.orbhip_grey(ex.handle, p(rgb), W, H, W * 3, M.FMT_RGBA, p(out), W))
    bad(L.orbhip_grey(ex.handle, p(rgb), W, H, W * 3, M.FMT_RGB, p(out), W - 1))
    bad(L.orbhip_extract_color(ex.handle, p(rgb), W, H, W * 3, M.FMT_BGRA, p(kps), p(desc), cap, C.byref(n), None))
    assert (out == POISON).all() and (desc == POISON).all() and n.value == -5
    # orbhip_grey_device: misaligned base, strides that are not multiples of 4
    d_src, d_dst = hiprt.DevBuf(W * H * 3 + 64), hiprt.DevBuf.from_numpy(np.full(W * H + 64, POISON, np.uint8))
    s, d = d_src.ptr.value, d_dst.ptr.value
    for args in ((s + 1, 1, W, H, W * 3, W * H * 3, M.FMT_RGB, d, W, W * H), (s, 1, W, H, W * 3, W * H * 3, M.FMT_RGB, d + 2, W, W * H),
                 (s, 1, W - 2, H, (W - 2) * 3, W * H * 3, M.FMT_RGB, d, W, W * H), (s, 1, W - 2, H, W * 3, W * H * 3, M.FMT_RGB, d, W - 2, W * H),
                 (s, 2, W, H // 2, W * 3, W * H * 3 // 2 + 2, M.FMT_RGB, d, W, W * H // 2), (s, 1, W, H, W * 3, W * H * 3, 7, d, W, W * H),
                 (s, 1, W, H, W * 3 - 4, W * H * 3, M.FMT_RGB, d, W, W * H), (s, 0, W, H, W * 3, W * H * 3, M.FMT_RGB, d, W, W * H)):
        bad(L.orbhip_grey_device(ex.handle, *args))
    ex.sync()
    assert (d_dst.to_numpy(np.uint8, (W * H + 64,)) == POISON).all()
    # orbhip_rgbd_depth_device: depth type, stride, alignment, factor
    depth = scenes.depth_map()
    d_depth, d_k = hiprt.DevBuf.from_numpy(depth), hiprt.DevBuf(cap * 28)
    d_ur = hiprt.DevBuf.from_numpy(ur)
    dp = d_depth.ptr.value
    for args in ((dp, 0, W, H, W * 2, 0, 0.5), (dp, 3, W, H, W * 2, 0, 0.5), (dp, rgbd.DEPTH_U16, W, H, W * 2 - 2, 0, 0.5),
                 (dp + 1, rgbd.DEPTH_U16, W, H, W * 2, 0, 0.5), (dp + 2, rgbd.DEPTH_F32, W // 2, H, W * 2, 0, 0.5),
                 (dp, rgbd.DEPTH_U16, W, H, W * 2 + 1, 0, 0.5), (dp, rgbd.DEPTH_U16, W, H, W * 2, 0, float("nan")),
                 (dp, rgbd.DEPTH_U16, W, H, W * 2, 0, float("-inf")), (None, rgbd.DEPTH_U16, W, H, W * 2, 0, 0.5)):
        bad(L.orbhip_rgbd_depth_device(ex.handle, d_k.ptr, d_k.ptr, None, cap, 1, *args, 40.0, d_ur.ptr, d_ur.ptr))
    ex.sync()
    assert (d_ur.to_numpy(f32, (cap,)) == 7).all()
    # orbhip_frame_build_rgbd: format, stride, depth type, depth stride, factor
    P = capi.FrameParams()
    for i, v in enumerate(np.eye(3, dtype=f32).ravel()):
        P.K[i] = float(v)
    P.levelsup = -1
    for over in (dict(format=9), dict(stride=W * 3 - 1), dict(depth_type=3), dict(depth_stride=W * 2 - 1), dict(depth_factor=float("inf")),
                 dict(depth=None)):
        I = rgbd.FrameInput(rgb.ctypes.data, W, H, W * 3, M.FMT_RGB, depth.ctypes.data, rgbd.DEPTH_U16, W * 2, 0.0002, 40.0)
        for k, v in over.items():
            setattr(I, k, v)
        bad(L.orbhip_frame_build_rgbd(ex.handle, C.byref(I), C.byref(P), p(kps), p(kun), p(desc), cap, C.byref(n), None, None, None, None,
                                      None, p(ur), p(dz)))
    assert (desc == POISON).all() and (ur == 7).all() and (dz == 7).all() and n.value == -5
    # without a depth map the two depth outputs may be NULL; with one they may not
    I = rgbd.FrameInput(rgb.ctypes.data, W, H, W * 3, M.FMT_RGB, None, rgbd.DEPTH_NONE, 0, 1.0, 40.0)
    assert L.orbhip_frame_build_rgbd(ex.handle, C.byref(I), C.byref(P), p(kps), p(kun), p(desc), cap, C.byref(n), None, None, None, None,
                                     None, None, None) == 0 and n.value > 100
    I = rgbd.FrameInput(rgb.ctypes.data, W, H, W * 3, M.FMT_RGB, depth.ctypes.data, rgbd.DEPTH_U16, W * 2, 0.0002, 40.0)
    bad(L.orbhip_frame_build_rgbd(ex.handle, C.byref(I), C.byref(P), p(kps), p(kun), p(desc), cap, C.byref(n), None, None, None, None,
                                  None, None, p(dz)))
    # the context still works
    g = M.grey(rgb, M.FMT_RGB)
    k, dd = rgbd.extract_color(ex, rgb, M.FMT_RGB)
    rk, rd = oracle.Extractor(1000)(g)
    assert k.tobytes() == rk.tobytes() and np.array_equal(dd, rd)
    assert np.array_equal(rgbd.grey(ex, rgb, M.FMT_RGB), g)
    for b in (d_src, d_dst, d_depth, d_k, d_ur):
        b.free()
