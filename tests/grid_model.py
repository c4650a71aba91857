"""Independent model of the frame grid and its window query: no device, no liborbhip, no oracle.  Written from the reference's
lines -- src/Frame.cc:574-589 AssignFeaturesToGrid, :726-736 PosInGrid, :671-724 GetFeaturesInArea -- with np.float32 scalars,
one rounding per float operation (the reference's members and arguments are floats; round / floor / ceil take the float
product widened to double, which is exact, and C's round() rounds halves away from zero).

The `variant` arguments compute what a wrong implementation would (the guard-scene convention of tests/correct_model.py):
tests/test_grid_model.py asserts that every one of them changes the result on at least one scene of tests/grid_scenes.py, which
is what shows that the scenes can see that bug.  Every function ignores the variants that are not its own, so a caller passes
the same variant to grid_build and to features_in_area.

Inputs are finite and of magnitude <= 1e6 (tests/grid_scenes.py): every float-to-int conversion below is defined."""
import math

import numpy as np

f32 = np.float32
COLS, ROWS = 64, 48
CELLS = COLS * ROWS

VARIANTS = ("half_even", "floor_cell", "le_radius", "no_grid", "narrow_window", "row_major", "cell_unsorted", "level_always")


def grid_params(min_x, max_x, min_y, max_y):
    """(mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv) -- src/Frame.cc:556-557."""
    return f32(min_x), f32(min_y), f32(COLS) / (f32(max_x) - f32(min_x)), f32(ROWS) / (f32(max_y) - f32(min_y))


def c_round(v):
    """C round() of a float widened to double: halves away from zero."""
    v = float(v)
    a = math.floor(abs(v) + 0.5)          # exact: |v| < 2^24 has room for the half in a double
    return int(-a if v < 0 else a)


def cell_coord(p, mn, inv):
    """(p - min) * inv as the reference computes it: two float operations."""
    return (f32(p) - f32(mn)) * f32(inv)


def pos_in_grid(x, y, gp, variant=None):
    """PosInGrid (:726-736): the cell id posX * 48 + posY, or -1 when the feature is not in the grid."""
    vx, vy = cell_coord(x, gp[0], gp[2]), cell_coord(y, gp[1], gp[3])
    if variant == "half_even":
        px, py = int(np.rint(vx)), int(np.rint(vy))
    elif variant == "floor_cell":
        px, py = math.trunc(float(vx)), math.trunc(float(vy))
    else:
        px, py = c_round(vx), c_round(vy)
    if px < 0 or px >= COLS or py < 0 or py >= ROWS:
        return -1
    return px * ROWS + py


def grid_build(kps, gp, variant=None):
    """AssignFeaturesToGrid (:574-589) as CSR: (off[3073], idx); a cell's entries in push_back order = ascending feature index."""
    cells = [[] for _ in range(CELLS)]
    xs, ys = kps["x"], kps["y"]
    for i in range(len(kps)):
        c = pos_in_grid(xs[i], ys[i], gp, variant)
        if c >= 0:
            cells[c].append(i)
    off = np.zeros(CELLS + 1, np.int32)
    idx = []
    for c in range(CELLS):
        idx.extend(reversed(cells[c]) if variant == "cell_unsorted" else cells[c])
        off[c + 1] = len(idx)
    return off, np.array(idx, np.int32)


def window_cells(gp, x, y, r, variant=None):
    """The cell window of GetFeaturesInArea (:676-690): (x0, x1, y0, y1), or None at one of the four early returns."""
    x, y, r = f32(x), f32(y), f32(r)
    if variant == "narrow_window":
        # The window's cells by a rounding conversion instead of floor / ceil.  The rounding is C's float-to-int conversion
        # (towards zero): it drops the last column and row whenever the high edge's cell coordinate has a fraction.  Rounding to
        # NEAREST is not used as the wrong variant because no scene can see it: a feature that passes the strict distance test
        # lies inside the window's edges, PosInGrid rounds its cell coordinate to nearest as well, and rounding is monotone -- its
        # cell is never outside the cells of the rounded edges (the reference's floor / ceil window is one cell wider than it
        # needs to be).  On the inexact grid the rounding of x - minX could in principle break the monotonicity; a random
        # search over some 10^8 windows around the cell boundaries found no such case.
        lo = hi = lambda v: math.trunc(float(v))
    else:
        lo, hi = (lambda v: math.floor(float(v))), (lambda v: math.ceil(float(v)))
    x0 = max(0, lo((x - gp[0] - r) * gp[2]))
    if x0 >= COLS:
        return None
    x1 = min(COLS - 1, hi((x - gp[0] + r) * gp[2]))
    if x1 < 0:
        return None
    y0 = max(0, lo((y - gp[1] - r) * gp[3]))
    if y0 >= ROWS:
        return None
    y1 = min(ROWS - 1, hi((y - gp[1] + r) * gp[3]))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def _passes(kps, i, x, y, r, min_level, max_level, variant):
    """The level filter (:705-712) and the distance test (:714-718) on feature i."""
    o = int(kps["octave"][i])
    if variant == "level_always":
        if o < min_level or o > max_level:
            return False
    elif min_level > 0 or max_level >= 0:
        if o < min_level:
            return False
        if max_level >= 0 and o > max_level:
            return False
    dx, dy = abs(f32(kps["x"][i]) - x), abs(f32(kps["y"][i]) - y)
    if variant == "le_radius":
        return bool(dx <= r and dy <= r)
    return bool(dx < r and dy < r)


def features_in_area(kps, grid, gp, x, y, r, min_level=-1, max_level=-1, variant=None):
    """GetFeaturesInArea (:671-724): the feature indices in the reference's visiting order (columns outer, rows inner, a
    cell's entries in stored order)."""
    x, y, r = f32(x), f32(y), f32(r)
    min_level, max_level = int(min_level), int(max_level)
    if variant == "no_grid":
        return [i for i in range(len(kps)) if _passes(kps, i, x, y, r, min_level, max_level, variant)]
    w = window_cells(gp, x, y, r, variant)
    if w is None:
        return []
    x0, x1, y0, y1 = w
    off, idx = grid
    if variant == "row_major":
        order = [(ix, iy) for iy in range(y0, y1 + 1) for ix in range(x0, x1 + 1)]
    else:
        order = [(ix, iy) for ix in range(x0, x1 + 1) for iy in range(y0, y1 + 1)]
    out = []
    for ix, iy in order:
        c = ix * ROWS + iy
        for j in range(int(off[c]), int(off[c + 1])):
            i = int(idx[j])
            if _passes(kps, i, x, y, r, min_level, max_level, variant):
                out.append(i)
    return out


def area(kps, gp, x, y, r, min_level=-1, max_level=-1, variant=None, grid=None):
    """grid_build + features_in_area with one variant for both."""
    if grid is None:
        grid = grid_build(kps, gp, variant)
    return features_in_area(kps, grid, gp, x, y, r, min_level, max_level, variant)


def column_records(grid, w):
    """Per window column x0..x1: the number of entries of its cells y0..y1 (what a device walker lays end to end)."""
    x0, x1, y0, y1 = w
    off = grid[0]
    return [int(off[c * ROWS + y1 + 1]) - int(off[c * ROWS + y0]) for c in range(x0, x1 + 1)]
