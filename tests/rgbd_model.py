"""Independent numpy model of the RGB-D sensor path, written from its definitions, not from the kernels:
grey conversion in plain int64 arithmetic, the depth lookup as np.float32 operations one at a time."""
import numpy as np

f32 = np.float32
FMT_GREY, FMT_RGB, FMT_BGR, FMT_RGBA, FMT_BGRA = range(5)
CHANNELS = {FMT_RGB: 3, FMT_BGR: 3, FMT_RGBA: 4, FMT_BGRA: 4}
CR, CG, CB = 4899, 9617, 1868


def grey(image, fmt):
    """(H, W, 3 or 4) uint8 -> (H, W) uint8: (4899 R + 9617 G + 1868 B + 8192) >> 14; the fourth channel is not looked at."""
    a = np.asarray(image).astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == CHANNELS[fmt]
    r, b = (a[:, :, 2], a[:, :, 0]) if fmt in (FMT_BGR, FMT_BGRA) else (a[:, :, 0], a[:, :, 2])
    v = (CR * r + CG * a[:, :, 1] + CB * b + 8192) >> 14
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def grey_tables(r, g, b):
    """OpenCV's table form: three 256-entry tables, the rounding bias inside the first, one shift."""
    i = np.arange(256, dtype=np.int64)
    tr, tg, tb = CR * i + 8192, CG * i, CB * i
    return (tr[r] + tg[g] + tb[b]) >> 14


def depth_at_keypoints(kps, kps_un, depth, factor, mbf):
    """(u_right, depth) per keypoint.  depth: (H, W) uint16 or float32; kps / kps_un: records with x, y."""
    d = np.asarray(depth)
    factor, mbf = f32(factor), f32(mbf)
    scales = d.dtype != np.float32 or abs(f32(factor - f32(1.0))) > f32(1e-5)
    n = len(kps)
    ur, dz = np.full(n, -1, f32), np.full(n, -1, f32)
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y = float(kps["x"][i]), float(kps["y"][i])
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            u, v = int(x), int(y)                   # truncation towards zero
            if u < 0 or v < 0 or u >= d.shape[1] or v >= d.shape[0]:
                continue                            # the stated divergence: outside the map = no depth
            z = f32(d[v, u])                        # uint16 -> float is exact
            if scales:
                z = f32(z * factor)
            if z > 0:                               # NaN fails
                dz[i] = z
                ur[i] = f32(f32(kps_un["x"][i]) - f32(mbf / z))
    return ur, dz
