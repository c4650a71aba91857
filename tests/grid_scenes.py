"""Constructed feature sets and window lists for the frame grid and every window walk built on it (tests/grid_model.py is the
model, tests/test_grid_model.py the CPU checks, tests/test_grid_edges_gpu.py the device checks).

RULE: every coordinate, radius and grid parameter in this file is finite and of magnitude at most 1e6, so that every
float-to-int conversion of the reference (src/Frame.cc:676-688, :728-729) is defined.  No NaN, no Inf, nothing larger: on such
inputs the reference's own conversion is undefined, the x86 oracle and the device differ, and nothing in the project specifies
the result.

Two grids: EXACT = grid_params(0, 512, 0, 384) -- both inverses are exactly 0.125, a cell is 8 pixels, column k holds
x in [8k - 4, 8k + 4) (column 0: (-4, 4)) -- and INEXACT = grid_params(22.5, 611.25, 19.75, 452.5), whose inverses are rounded."""
import functools

import numpy as np

import grid_model as M

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
EXACT = M.grid_params(0, 512, 0, 384)
INEXACT = M.grid_params(22.5, 611.25, 19.75, 452.5)
LIMIT = 1e6

LEVEL_FILTERS = [(-1, -1), (0, -1), (0, 0), (0, 3), (2, -1), (3, 4)]
# the thread and wave boundaries of k_grid_build's cell ranges: PER = 3 (1024 threads) and 12 (256 threads) cells per thread,
# 192 and 768 per wave; and the two ends of the grid
EDGE_CELLS = [0, 2, 3, 11, 12, 191, 192, 767, 768, 3071]


def make_kps(x, y, octave=0):
    x = np.asarray(x, f32).ravel()
    k = np.zeros(len(x), KP_DTYPE)
    k["x"], k["y"], k["octave"] = x, np.asarray(y, f32), octave
    k["size"], k["class_id"] = 31, -1
    assert np.isfinite(k["x"]).all() and np.isfinite(k["y"]).all()
    assert (np.abs(k["x"]) <= LIMIT).all() and (np.abs(k["y"]) <= LIMIT).all()
    return k


def step(v, n):
    """v moved n float32 steps (n < 0: towards -inf)."""
    v = f32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, f32(np.inf if n > 0 else -np.inf))
    return v


def cell_points(col, row, m):
    """m distinct positions inside cell (col, row) of the EXACT grid, at most 3.25 pixels from its centre."""
    j = np.arange(m)
    dx = -3 + (j % 13) * 0.5 + 0.25 * (j // 169)
    dy = -3 + ((j // 13) % 13) * 0.5
    return (8 * col + dx).astype(f32), (8 * row + dy).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# cell scenes: dict(name, kps, gp)
# ---------------------------------------------------------------------------------------------------------------------

def _half_coords(last):
    """Cell coordinates on and around k + 0.5, the two borders and small negatives (last = 63 for columns, 47 for rows)."""
    c = [-0.75, -0.5, step(-0.5, 1), -0.25, -0.0, 0.0, 0.25, step(0.5, -1), 0.5, 1.5, 2.5, 3.5, 10.5, 21.5, last - 0.5,
         step(last + 0.5, -1), last + 0.5, last + 0.75, last + 1.0]
    return np.array(c, f32)


def _inexact_near_half(mn, inv, last):
    """Coordinates of the INEXACT grid whose cell coordinate lies within two float steps of k + 0.5."""
    out = []
    for k in (-1, 0, 1, 2, 7, 30, last - 1, last):
        p = f32(f32(mn) + f32(k + 0.5) / f32(inv))
        out += [step(p, d) for d in (-2, -1, 0, 1, 2)]
    return np.array(out, f32)


def _generic(n, gp, seed):
    """n features over the grid and a margin around it, some cells with several entries; the features of a cell lie far apart in
    the index order."""
    rng = np.random.default_rng(seed)
    w, h = f32(64) / gp[2], f32(48) / gp[3]
    x = gp[0] + rng.uniform(-0.08, 1.08, n) * w
    y = gp[1] + rng.uniform(-0.08, 1.08, n) * h
    if n >= 64:                         # 16 clusters of features that share a cell, their indices spread over the whole range
        for c in range(16):
            members = (c * 7 + np.arange(1 + c % 5) * (n // 5 + 3)) % n
            x[members], y[members] = x[members[0]], y[members[0]]
    return make_kps(x, y, rng.integers(0, 8, n))


def _multi(m):
    """2100 features; every cell of EDGE_CELLS holds m of them, their indices interleaved over the threads of k_grid_build
    (i, i + 2050, i + 260, i + 1030, ...: below and above 256, 1024 and 2048, the features a thread keeps in registers and the
    ones it loops over); the rest one per cell elsewhere, or outside."""
    n = 2100
    x, y = np.zeros(n, f32), np.zeros(n, f32)
    used = np.zeros(n, bool)
    offs = [0, 2050, 260, 1030, 520, 1540, 780, 1290]
    for e, cell in enumerate(EDGE_CELLS):
        px, py = cell_points(cell // 48, cell % 48, m)
        for j in range(m):
            i = (5 * e + offs[j % 8] + 61 * (j // 8)) % n
            while used[i]:
                i = (i + 1) % n
            used[i] = True
            x[i], y[i] = px[j], py[j]
    free = np.nonzero(~used)[0]
    for t, i in enumerate(free):
        cell = 1000 + 13 * ((t * 37) % len(free))   # single-entry cells away from EDGE_CELLS; beyond the grid: outside
        x[i], y[i] = 8 * (cell // 48) + 1, 8 * (cell % 48) - 1
    return make_kps(x, y, np.arange(n) % 8)


def cell_scenes():
    S = []
    cx, cy = _half_coords(63), _half_coords(47)
    S.append(dict(name="half_x_exact", gp=EXACT, kps=make_kps(cx * 8, np.full(len(cx), 41.0))))
    S.append(dict(name="half_y_exact", gp=EXACT, kps=make_kps(np.full(len(cy), 54.0), cy * 8)))
    S.append(dict(name="half_xy_exact", gp=EXACT, kps=make_kps(np.concatenate([cx, cx[::-1]]) * 8,
                                                                np.concatenate([cy, cy]) * 8)))
    ix = _inexact_near_half(INEXACT[0], INEXACT[2], 63)
    iy = _inexact_near_half(INEXACT[1], INEXACT[3], 47)
    S.append(dict(name="near_half_x_inexact", gp=INEXACT, kps=make_kps(ix, np.full(len(ix), 100.0))))
    S.append(dict(name="near_half_y_inexact", gp=INEXACT, kps=make_kps(np.full(len(iy), 100.0), iy)))
    far = [(-1e6, 100), (1e6, 100), (100, -1e6), (100, 1e6), (-1e6, -1e6), (1e6, 1e6), (-100, 100), (700, 100), (100, -100),
           (100, 500), (100, 100), (300, 200), (-3.99, 0), (-4, 0), (508, 0), (507.99, 0), (4, 4), (12, 12), (20, 20)]
    for gname, gp in (("exact", EXACT), ("inexact", INEXACT)):
        S.append(dict(name="far_outside_" + gname, gp=gp, kps=make_kps([p[0] for p in far], [p[1] for p in far])))
    for m in (2, 3, 17, 200):
        S.append(dict(name="multi_%d" % m, gp=EXACT, kps=_multi(m)))
    for n in (0, 1, 2047, 2048, 2049, 2100):
        S.append(dict(name="n%d_exact" % n, gp=EXACT, kps=_generic(n, EXACT, 100 + n)))
        S.append(dict(name="n%d_inexact" % n, gp=INEXACT, kps=_generic(n, INEXACT, 200 + n)))
    px, py = cell_points(17, 29, 200)
    perm = np.random.default_rng(5).permutation(200)
    S.append(dict(name="one_cell_200", gp=EXACT, kps=make_kps(px[perm], py[perm], perm % 8)))
    S.append(dict(name="all_outside", gp=EXACT, kps=make_kps(np.linspace(-900, -10, 50), np.linspace(400, 900, 50))))
    return S


# ---------------------------------------------------------------------------------------------------------------------
# window scenes: dict(name, kps, gp, windows = [(x, y, r, min_level, max_level), ...])
# ---------------------------------------------------------------------------------------------------------------------

def from_occupancy(occ, extra=(), seed=1):
    """Features of the EXACT grid from occ = [(col, row, count, octave function of j)], plus extra = [(x, y, octave)], in a fixed
    shuffled index order (so that ascending index is not the visiting order)."""
    xs, ys, os_ = [], [], []
    for col, row, m, fo in occ:
        px, py = cell_points(col, row, m)
        xs += list(px)
        ys += list(py)
        os_ += [fo(j) for j in range(m)]
    for x, y, o in extra:
        xs.append(x)
        ys.append(y)
        os_.append(o)
    perm = np.random.default_rng(seed).permutation(len(xs))
    return make_kps(np.array(xs, f32)[perm], np.array(ys, f32)[perm], np.array(os_, np.int32)[perm])


def span_window(k, ncols, y):
    """(x, r) of a window of the EXACT grid over exactly the columns k .. k + ncols - 1 (ncols >= 2), whose low edge has cell
    coordinate k + 0.25 and whose high edge k + ncols - 1.25: the outermost columns can hold features that pass."""
    return f32(8 * k + 4 * ncols - 4), f32(y), f32(4 * ncols - 6)


def _scene_spans():
    """Every column holds features at rows 10, 20 and 30 (13 each in the corner columns), two in the last cell, some outside."""
    occ = []
    for c in range(64):
        for row in (10, 20, 30):
            m = 13 if c in (0, 63) and row == 20 else 1
            occ.append((c, row, m, lambda j, c=c, row=row: (c + row // 10 + j) % 8))
    occ.append((63, 47, 2, lambda j: j))
    extra = [(-10, 160, 0), (-6, 158, 1), (520, 160, 2), (516, 161, 0), (256, -10, 3), (256, 390, 0), (250, -5, 0)]
    kps = from_occupancy(occ, extra, seed=2)
    W = []
    y = 160
    W.append((-4.5, y, 4))                       # 1 column (clamped at the left border)
    W.append((508.5, y, 4))                      # 1 column (clamped at the right border)
    W += [(8 * 20, y, 50), (8 * 20 + 4, y, 58), (8 * 20, y, 58), (8 * 30 + 4, y, 122), (8 * 31, y, 122), (256, y, 300),
          (252, y, 250)]                         # 15, 16, 17, 32, 33, 64 (clamped), 64 columns
    W += [span_window(10, n, y) for n in (2, 15, 16, 17, 32, 33)]
    W += [(500, 380, 20), (505, 376, 9)]         # reach column 63 and row 47: the sentinel off[3072] is read
    W += [(600, y, 50), (-100, y, 50), (256, 500, 50), (256, -100, 50)]      # the four early returns
    W += [(-20, y, 40), (520, y, 40), (256, -20, 40), (256, 400, 40), (-8, -8, 30), (515, 388, 30)]   # partly outside
    windows = [(x, yy, r, -1, -1) for x, yy, r in W]
    for mn, mx in LEVEL_FILTERS:                 # the level filters on a many-column and on a one-column window
        windows += [(8 * 31, y, 122, mn, mx), (-4.5, y, 4, mn, mx), (256, 192, 300, mn, mx)]
    return dict(name="spans", gp=EXACT, kps=kps, windows=windows)


def _scene_chunks():
    """Record totals per 16-column chunk.  Row 2: chunk 0 holds 15 records with empty columns at both ends, chunk 1 none,
    chunk 2 sixteen, column 48 seventeen.  Row 40: 63, 64 and 65 records in chunks 0, 1, 2 and an empty last column."""
    occ = []
    for c in range(2, 15):
        occ.append((c, 2, 3 if c == 7 else 1, lambda j, c=c: (c + j) % 8))
    for c in range(32, 48):
        occ.append((c, 2, 1, lambda j, c=c: c % 8))
    occ.append((48, 2, 17, lambda j: j % 8))
    for c in range(48):
        m = 3 if c == 0 else (5 if c == 32 else 4)
        occ.append((c, 40, m, lambda j, c=c: (c + 2 * j) % 8))
    kps = from_occupancy(occ, seed=3)
    windows = []
    for y in (16, 368):
        windows += [(192, y, 186, mn, mx) for mn, mx in [(-1, -1), (0, 0), (3, 4)]]
        windows += [(8 * 24 + 4, y, 186, -1, -1), (8 * 8, y, 58, -1, -1), (8 * 40, y, 90, 0, 3)]
    return dict(name="chunks", gp=EXACT, kps=kps, windows=windows)


def cluster_radius(k):
    """Radius at which a window on the cluster's centre holds exactly k of its 129 level-0 features (k = 0 .. 129)."""
    return f32(2 + 0.25 * k - 0.125) if k <= 128 else f32(34.125)


CLUSTER_CENTRE = (f32(256), f32(192))
CLUSTER_COUNTS = (0, 1, 16, 17, 32, 33, 64, 65, 128, 129)


def _scene_cluster():
    """129 level-0 features around (256, 192), feature j at Chebyshev distance exactly 2 + j / 4 from it, on alternating sides;
    features of octaves 1..7 among them.  A window of radius cluster_radius(k) holds exactly k level-0 features."""
    cx, cy = CLUSTER_CENTRE
    extra = []
    for j in range(129):
        rho = 2 + 0.25 * j
        u = np.round(rho * (((j * 37) % 21) - 10) / 11 * 64) / 64
        x, y = [(cx + rho, cy + u), (cx - rho, cy + u), (cx + u, cy + rho), (cx + u, cy - rho)][j % 4]
        extra.append((x, y, 0))
        if j % 3 == 0:
            extra.append((x + 0.125 if j % 4 >= 2 else x, y + 0.125 if j % 4 < 2 else y, 1 + j % 7))
    kps = from_occupancy([], extra, seed=4)
    windows = [(cx, cy, cluster_radius(k), 0, 0) for k in CLUSTER_COUNTS]
    windows += [(cx, cy, cluster_radius(k), mn, mx) for k in (17, 64, 129) for mn, mx in LEVEL_FILTERS]
    return dict(name="cluster", gp=EXACT, kps=kps, windows=windows)


def _scene_radius_edges(gp, name):
    """Features exactly on |dx| = r and |dy| = r and one float step inside, at both ends (the low end lies in r's binade: its
    inside neighbour is exactly one step of r inside)."""
    x, y, r = f32(100), f32(100), f32(37.5)
    extra = []
    for e in (x - r, x + r):
        extra += [(step(e, d), y + f32(d), 0) for d in (-2, -1, 0, 1, 2)]
    for e in (y - r, y + r):
        extra += [(x + f32(d), step(e, d), 0) for d in (-2, -1, 0, 1, 2)]
    extra += [(step(x - r, 1), step(y - r, 1), 0), (x + r, y, 0), (x, y, 0), (step(x + r, -1), step(y + r, -1), 0)]
    return dict(name=name, gp=gp, kps=from_occupancy([], extra, seed=5), windows=[(x, y, r, -1, -1), (x, y, r, 0, 3)])


def _scene_outer_cells():
    """Features one float step inside each edge of windows whose edges have cell-coordinate fractions .25 and .75 in every
    combination: with .25 at the low end / .75 at the high end the feature's cell is the outermost cell of the floor / ceil
    range -- a window narrowed by one cell loses it."""
    wins = [(144, 144, 62), (148, 148, 62), (146, 146, 64), (150, 150, 64), (144, 150, 62), (148, 146, 64)]
    extra = []
    for i, (x, y, r) in enumerate(wins):
        x, y, r = f32(x), f32(y), f32(r)
        extra += [(step(x - r, 1), y, i % 8), (step(x + r, -1), y + 1, i % 8), (x, step(y - r, 1), i % 8),
                  (x + 1, step(y + r, -1), i % 8), (x - r, y - 1, 0), (x + 2, y + r, 0)]
    return dict(name="outer_cells", gp=EXACT, kps=from_occupancy([], extra, seed=6),
                windows=[(x, y, r, -1, -1) for x, y, r in wins])


def _scene_inexact():
    """The window query on the INEXACT grid: generic features, windows on a lattice of centres and radii, all level filters."""
    kps = _generic(600, INEXACT, 77)
    windows = []
    for i, x in enumerate((-30, 22.5, 100.3, 316.9, 611.25, 650)):
        for j, y in enumerate((-20, 19.75, 236.1, 452.5, 480)):
            mn, mx = LEVEL_FILTERS[(i + j) % 6]
            windows.append((x, y, (3, 17.5, 60, 250)[(i + 2 * j) % 4], mn, mx))
    return dict(name="generic_inexact", gp=INEXACT, kps=kps, windows=windows)


def window_scenes():
    S = [_scene_spans(), _scene_chunks(), _scene_cluster(), _scene_radius_edges(EXACT, "radius_edges_exact"),
         _scene_radius_edges(INEXACT, "radius_edges_inexact"), _scene_outer_cells(), _scene_inexact()]
    for s in S:
        w = np.array(s["windows"], np.float64)
        assert np.isfinite(w).all() and (np.abs(w) <= LIMIT).all()
    return S


# ---------------------------------------------------------------------------------------------------------------------
# projection scenes: one window each, the candidates placed column by column.  dict(name, kps, gp, window, count)
# ---------------------------------------------------------------------------------------------------------------------

def _columns_scene(name, k, ncols, per_col, y=160, distract=True):
    """A window over the columns k .. k + ncols - 1; per_col[c] level-0 features that pass in column k + c; features of octave
    5 beside them and level-0 features in the window's cells beyond the radius in y (records that do not pass)."""
    x, y, r = span_window(k, ncols, y)
    extra = []
    for c, m in enumerate(per_col):
        dx = 3 if c == 0 else (-3 if c == ncols - 1 else 0)       # the outermost columns: just inside the window's edge
        for j in range(m):
            # over five rows of cells where the radius allows it: columns outer, rows inner is then not the order of y alone
            extra.append((8 * (k + c) + dx, y + ((c * 3 + j * 5) % 7 - 3) * (4.0 if r >= 16 else 0.5) + 0.0625 * j, 0))
        if m and distract:
            extra.append((8 * (k + c) + dx, y + 0.5, 5))
            row0 = int(np.floor((y - r) / 8))
            if row0 >= 0:
                extra.append((8 * (k + c) + dx, 8 * row0 - 3, 0))   # in the window's first row of cells, outside the radius
    mid = 8 * (k + int(np.argmax(per_col))) + 1
    extra += [(mid, y + r, 0), (mid + 0.5, y - r, 0), (x + r, y, 0), (x - r, y + 1, 0)]      # exactly on the radius: not candidates
    return dict(name=name, gp=EXACT, kps=from_occupancy([], extra, seed=10 + ncols), window=(x, y, r, 0, 0),
                count=int(sum(per_col)), ncols=ncols)


def proj_scenes():
    S = [_columns_scene("c2_n1", 5, 2, [1, 0]),
         _columns_scene("c16_n16", 10, 16, [1] * 16),
         _columns_scene("c17_n17", 10, 17, [1] * 17),
         _columns_scene("c17_n16_last", 20, 17, [15] + [0] * 15 + [1]),                 # the 16th candidate alone in chunk 1
         _columns_scene("c32_n17_gaps", 8, 32, [0, 0, 3] + [1] * 6 + [0] * 7 + [0, 1, 1] + [1] * 6 + [0] * 7),
         _columns_scene("c33_n32_empty_chunk", 12, 33, [2] * 15 + [1] + [0] * 16 + [1]),   # chunk 1 wholly empty
         _columns_scene("c33_n33", 12, 33, [1] * 33),
         _columns_scene("c17_n33", 30, 17, [2] * 16 + [1])]
    # one column, clamped at the border; sixteen candidates in (-4, -0.5), one feature outside the grid within the radius
    extra = [(-3.9 + 0.2 * j, 160 + (j % 5) - 2, 0) for j in range(16)] + [(-6, 160, 0), (-2, 161, 4), (2, 160, 0)]
    S.append(dict(name="c1_n16_border", gp=EXACT, kps=from_occupancy([], extra, seed=30), window=(f32(-4.5), f32(160), f32(4), 0, 0),
                  count=16, ncols=1))
    # reaches column 63 and row 47
    extra = [(505, 379, 0), (503, 377.5, 0), (501, 376, 3), (509, 378, 0), (490, 360, 0)]
    S.append(dict(name="c_last_n2", gp=EXACT, kps=from_occupancy([], extra, seed=31), window=(f32(506), f32(378), f32(5), 0, 0),
                  count=2, ncols=2))
    return S


# ---------------------------------------------------------------------------------------------------------------------
# initialisation scenes: frame 2's features and one window (integer radius); count level-0 features pass
# ---------------------------------------------------------------------------------------------------------------------

def _init_scene(name, x, y, r, count, ncols, lo=None, hi=None):
    """count level-0 features spread evenly over the passing range of x (lo, hi), octave-1 features among them, level-0
    features exactly on the radius and, where the grid allows, outside the grid but within the radius."""
    lo = x - r + 0.5 if lo is None else lo
    hi = x + r - 0.5 if hi is None else hi
    xs = np.round(np.linspace(lo, hi, count) * 64) / 64 if count > 1 else np.array([np.round((lo + hi) * 32) / 64])
    amp = 4 if r >= 16 else 1                                # over five rows of cells where the radius allows it
    extra = [(xs[j], y + ((j * 5) % 7 - 3) * amp, 0) for j in range(count)]
    extra += [(xs[j], y + 0.125, 1 + j % 3) for j in range(0, count, 4)]
    extra += [(xs[0], y + r, 0), (xs[-1], y - r, 0)]
    if x + r < 500:
        extra.append((x + r, y, 0))
    if x - r < -4:
        extra.append((max(x - r + 1, -30), y, 0))          # outside the grid, within the radius
    return dict(name=name, gp=EXACT, kps=from_occupancy([], extra, seed=40 + count + ncols), window=(f32(x), f32(y), int(r)),
                count=count, ncols=ncols)


def init_scenes():
    S = []
    for count in (1, 64):
        S.append(_init_scene("c1_n%d" % count, -4.5, 160, 4, count, 1, lo=-3.9, hi=-0.6))
    for count in (63, 65):
        S.append(_init_scene("c16_n%d" % count, 8 * 20 + 4, 160, 58, count, 16))
    S.append(_init_scene("c17_n128", 8 * 20, 160, 58, 128, 17))
    for count in (64, 129):
        S.append(_init_scene("c63_n%d" % count, 248, 200, 242, count, 63))
    for count in (1, 65):
        S.append(_init_scene("c64_n%d" % count, 252, 200, 250, count, 64))
    return S


# ---------------------------------------------------------------------------------------------------------------------
# the constructions that make the visiting order observable through the matchers (expected values from the model only)
# ---------------------------------------------------------------------------------------------------------------------

QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("proj_xr", "<f4"), ("min_level", "<i4"),
                        ("max_level", "<i4"), ("angle", "<f4"), ("flags", "<i4")])
Q_ACTIVE, Q_OBSERVED = 1, 2
PROJ_XR = f32(100)


def stereo_u_right(kps, order, r):
    """mvuRight for a projection scene: the first candidates of the visiting order get a right coordinate exactly on
    |proj_xr - u_right| = r (kept: the reference drops only > r, src/ORBmatcher.cc:92-97), one float step beyond (dropped), at
    both ends, -1 and 0 (no right coordinate: not checked); every other feature one pixel off.  Returns (u_right, kept order)."""
    ur = np.full(len(kps), PROJ_XR + f32(1), f32)
    special = [PROJ_XR + f32(r), step(PROJ_XR + f32(r), 1), f32(-1), PROJ_XR - f32(r), step(PROJ_XR - f32(r), -1), f32(0)]
    for i, v in zip(order, special):
        ur[i] = v
    kept = [i for i in order if not (ur[i] > 0 and abs(PROJ_XR - ur[i]) > f32(r))]
    return ur, kept


def proj_case(scene, order, stereo=False):
    """SearchByProjection inputs for one projection scene and what the reference returns: every descriptor equal, len(order) + 2
    identical ACTIVE | OBSERVED queries, use_ratio = check_ori = False -- query i takes the i-th candidate of the visiting order
    (each closes its feature), the last two find nothing.  order = the model's list for scene['window']."""
    kps = scene["kps"]
    x, y, r, mn, mx = scene["window"]
    ur = None
    if stereo:
        ur, order = stereo_u_right(kps, order, r)
    nq = len(order) + 2
    q = np.zeros(nq, QUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["proj_xr"], q["min_level"], q["max_level"] = x, y, r, PROJ_XR, mn, mx
    q["flags"] = Q_ACTIVE | Q_OBSERVED
    match = np.full(len(kps), -1, np.int32)
    match[np.array(order, np.int64)] = np.arange(len(order))
    return dict(kps=kps, desc=np.full((len(kps), 32), 0x5A, np.uint8), q=q, qd=np.full((nq, 32), 0x5A, np.uint8), u_right=ur,
                match=match, n=len(order))


def init_case(scene, order):
    """SearchForInitialization inputs for one initialisation scene and what the reference returns: frame 1 = len(order) + 2
    level-0 features with all-zero descriptors and the same vbPrevMatched (the window's centre); every descriptor of frame 2 has
    one bit set (distance 1); nnratio = 2, check_ori = False -- feature i takes the i-th level-0 candidate of the visiting order
    (a matched feature of frame 2 is skipped by the next one: vMatchedDistance <= 1), the last two find nothing.
    order = the model's list for the window with levels (0, 0)."""
    kps2 = scene["kps"]
    x, y, r = scene["window"]
    n1 = len(order) + 2
    kps1 = make_kps(np.full(n1, 10.0) + np.arange(n1), np.full(n1, 20.0), 0)
    d2 = np.zeros((len(kps2), 32), np.uint8)
    d2[np.arange(len(kps2)), np.arange(len(kps2)) % 32] = 1 << (np.arange(len(kps2)) % 7)
    m12 = np.full(n1, -1, np.int32)
    m12[:len(order)] = order
    prev = np.tile(np.array([x, y], f32), (n1, 1))
    prev_after = prev.copy()
    for i, f in enumerate(order):
        prev_after[i] = kps2["x"][f], kps2["y"][f]
    return dict(kps1=kps1, d1=np.zeros((n1, 32), np.uint8), kps2=kps2, d2=d2, prev=prev, window_size=int(r), m12=m12,
                n=len(order), prev_after=prev_after)


@functools.lru_cache(maxsize=None)
def modelled():
    """Every scene with the model's grid ('grid') and, for the scenes with windows, the model's lists ('windows', 'lists'):
    computed once per process and shared by the tests; nobody changes it."""
    cells, wins, proj, init = cell_scenes(), window_scenes(), proj_scenes(), init_scenes()
    for s in cells + wins + proj + init:
        s["grid"] = M.grid_build(s["kps"], s["gp"])
    for s in proj:
        s["windows"] = [s["window"]]
    for s in init:
        x, y, r = s["window"]
        s["windows"] = [(x, y, f32(r), 0, 0)]
    for s in wins + proj + init:
        s["lists"] = [M.features_in_area(s["kps"], s["grid"], s["gp"], *w) for w in s["windows"]]
    return dict(cells=cells, wins=wins, proj=proj, init=init)
