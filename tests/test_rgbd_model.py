"""The RGB-D path's arithmetic on the CPU: known answers of the model (tests/rgbd_model.py), the table form of the grey
conversion against the multiply form on all 2^24 colours, the model against Pillow, and the library's host gather
(orbhip_rgbd_depth needs no device) against the model, by float bit patterns."""
import numpy as np
import pytest

import rgbd_model as M

f32 = np.float32


def _px(*rgb):
    return np.array([[list(rgb)]], np.uint8)


def test_grey_known_answers():
    assert M.grey(_px(0, 0, 0), M.FMT_RGB)[0, 0] == 0
    assert M.grey(_px(255, 255, 255), M.FMT_RGB)[0, 0] == 255
    assert [int(M.grey(_px(*c), M.FMT_RGB)[0, 0]) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [76, 150, 29]
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(M.grey(rgb[:, :, ::-1], M.FMT_BGR), M.grey(rgb, M.FMT_RGB))
    assert [int(M.grey(_px(*c), M.FMT_BGR)[0, 0]) for c in ((255, 0, 0), (0, 0, 255))] == [29, 76]
    # alpha is ignored
    for a in (0, 7, 255):
        rgba = np.dstack([rgb, np.full(rgb.shape[:2], a, np.uint8)])
        assert np.array_equal(M.grey(rgba, M.FMT_RGBA), M.grey(rgb, M.FMT_RGB))
        bgra = np.dstack([rgb[:, :, ::-1], rng.integers(0, 256, rgb.shape[:2], dtype=np.uint8)])
        assert np.array_equal(M.grey(bgra, M.FMT_BGRA), M.grey(rgb, M.FMT_RGB))


def test_table_form_equals_multiply_form_on_every_colour():
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    top = 0
    for r in range(256):
        rr = np.full_like(g, r)
        mul = (M.CR * rr.astype(np.int64) + M.CG * g + M.CB * b + 8192) >> 14
        assert np.array_equal(M.grey_tables(rr, g, b), mul)
        top = max(top, int(mul.max()))
    assert top == 255 and 255 * (M.CR + M.CG + M.CB) + 8192 == 255 * 16384 + 8192   # the weights sum to 2^14: nothing saturates


def test_model_against_pillow():
    """Pillow's L = (19595 R + 38470 G + 7471 B + 32768) >> 16: weights within (1, 2, 1) / 65536 of 4 x ours, so the unrounded
    values differ by less than 0.008 and the results by one level at the most."""
    Image = pytest.importorskip("PIL.Image")
    from orbhip import synth
    images = synth.load_photographs_rgb() + [np.random.default_rng(3).integers(0, 256, (240, 320, 3), dtype=np.uint8)]
    for rgb in images:
        pil = np.asarray(Image.fromarray(rgb, "RGB").convert("L")).astype(np.int32)
        diff = np.abs(M.grey(rgb, M.FMT_RGB).astype(np.int32) - pil)
        print("%d x %d: %.4f %% of the pixels differ from Pillow by one level" % (rgb.shape[1], rgb.shape[0], 100.0 * (diff != 0).mean()))
        assert diff.max() <= 1


def _kps(xy):
    from orbhip.capi import KP_DTYPE
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = np.asarray(xy, f32)[:, 0], np.asarray(xy, f32)[:, 1]
    return k


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def test_depth_known_answers():
    factor = f32(1.0) / f32(5000.0)
    d16 = np.zeros((4, 6), np.uint16)
    d16[1, 2], d16[2, 3] = 5000, 0
    kp, kun = _kps([(2.9, 1.9), (3.2, 2.0), (5.99, 3.99), (6.0, 1.0), (2.0, 4.0), (-0.5, 0.5)]), _kps([(2.5, 0)] * 6)
    ur, dz = M.depth_at_keypoints(kp, kun, d16, factor, 40.0)
    want = f32(f32(5000.0) * factor)               # the float product, whatever it is
    assert _bits(dz)[0] == _bits(want) and _bits(ur)[0] == _bits(f32(f32(2.5) - f32(f32(40.0) / want)))
    assert abs(float(want) - 1.0) < 1e-6
    for i in (1, 2, 3, 4):                          # raw 0 (twice), x = w, y = h
        assert (ur[i], dz[i]) == (-1, -1), i
    assert (ur[5], dz[5]) == (-1, -1)               # (int)-0.5 = 0 is inside; the pixel there is 0
    d32 = np.array([[np.nan, -1.0, 2.0, 0.0]], f32)
    kp, kun = _kps([(0, 0), (1, 0), (2, 0), (3, 0)]), _kps([(100.0, 0)] * 4)
    ur, dz = M.depth_at_keypoints(kp, kun, d32, 1.0, 40.0)
    assert list(dz) == [-1, -1, 2, -1] and list(ur) == [-1, -1, 80, -1]
    # 1 + 5e-6 is within 1e-5 of 1: the map is passed through unmultiplied
    near = f32(1.0) + f32(5e-6)
    assert near != f32(1.0)
    odd = np.array([[f32(3.3333333)]], f32)
    ur, dz = M.depth_at_keypoints(_kps([(0, 0)]), _kps([(9.0, 0)]), odd, near, 40.0)
    assert _bits(dz)[0] == _bits(odd[0, 0]) and _bits(f32(odd[0, 0] * near)) != _bits(odd[0, 0])
    ur, dz = M.depth_at_keypoints(_kps([(0, 0)]), _kps([(9.0, 0)]), odd, 0.5, 40.0)
    assert _bits(dz)[0] == _bits(f32(odd[0, 0] * f32(0.5)))
    # a uint16 map is always multiplied, also by a factor next to 1
    ur, dz = M.depth_at_keypoints(_kps([(2, 1)]), _kps([(9.0, 0)]), d16, near, 40.0)
    assert _bits(dz)[0] == _bits(f32(f32(5000.0) * near))


def _random_case(rng, dtype, n=4000, w=97, h=61):
    if dtype == np.uint16:
        d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < 0.2] = 0
    else:
        d = (rng.random((h, w)) * 9 - 1).astype(f32)
        d[rng.random((h, w)) < 0.05] = np.nan
        d[rng.random((h, w)) < 0.05] = 0
        d[rng.random((h, w)) < 0.02] = np.inf
    xy = np.stack([rng.random(n) * (w + 4) - 2, rng.random(n) * (h + 4) - 2], 1).astype(f32)
    xy[:8] = [(w, 3), (3, h), (w - 0.25, h - 0.25), (-0.75, 2), (2, -0.75), (-1, 2), (np.nan, 2), (1e20, 2)]
    kun = _kps(xy + rng.standard_normal((n, 2)).astype(f32) * 3)
    return _kps(xy), kun, d


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("factor", [1.0 / 5000.0, 1.0, 1.0 + 5e-6, 0.5, 1.0 + 2e-5])
def test_library_host_gather_equals_the_model(dtype, factor):
    """orbhip_rgbd_depth runs on the host and takes no context: the same three float operations, bit for bit."""
    from orbhip import rgbd
    kp, kun, d = _random_case(np.random.default_rng(11), dtype)
    # a strided map: the lookup honours depth_stride
    wide = np.zeros((d.shape[0], d.shape[1] + 5), d.dtype)
    wide[:, :d.shape[1]] = d
    for depth in (d, wide[:, :d.shape[1]]):
        ur, dz = rgbd.rgbd_depth(kp, kun, depth, f32(factor), 40.0)
        mur, mdz = M.depth_at_keypoints(kp, kun, d, f32(factor), 40.0)
        assert np.array_equal(_bits(dz), _bits(mdz)) and np.array_equal(_bits(ur), _bits(mur))
    assert (mdz > 0).sum() > 500 and (mdz < 0).sum() > 500


def test_library_host_gather_rejects_bad_arguments():
    from orbhip import capi, rgbd
    L = capi.load()
    kp, kun, d = _random_case(np.random.default_rng(2), np.uint16, n=10)
    ur, dz = np.full(10, 7, f32), np.full(10, 7, f32)

    def call(depth_type=rgbd.DEPTH_U16, stride=d.strides[0], factor=0.5, ptr=d.ctypes.data):
        return L.orbhip_rgbd_depth(None, kp.ctypes.data, kun.ctypes.data, 10, ptr, depth_type, d.shape[1], d.shape[0], stride, factor,
                                   40.0, ur.ctypes.data, dz.ctypes.data)
    for bad in (dict(depth_type=0), dict(depth_type=3), dict(stride=d.shape[1] * 2 - 1), dict(factor=float("nan")),
                dict(factor=float("inf")), dict(ptr=None)):
        assert call(**bad) == -1 and capi.last_error(None)
        assert (ur == 7).all() and (dz == 7).all()
    assert call() == 0 and not (dz == 7).any()
