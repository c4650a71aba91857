"""Constructed scenes for ORBmatcher::SearchForInitialization (tests/init_search_model.py is the model,
tests/test_init_search_model.py the CPU checks, tests/test_init_search_edges_gpu.py the device checks).

A scene is a dict of name, k1, d1, k2, d2, gp, prev, window, nnratio, check_ori, and ix = the rows of frame 1 it is about.
Dependency scenes carry dep = dict(drop, rows, changes): taking feature `drop` out of frame 1 changes the result of `rows`
(changes = True) or, for the counter-cases, of no row.  Ladder scenes carry lad = the claims the trace has to confirm.

Everything lies on the grid of grid_params(0, 512, 0, 384): both inverses are exactly 0.125 and a cell is 8 pixels.  Coordinates
and angles are exact in float32.  Every Hamming distance is known by construction: a frame-2 feature has `w` bits set among the
bits 0..127, a frame-1 feature has `t` bits set among the bits 128..255, so their distance is w + t; WHICH frame-2 features a
frame-1 feature sees is decided by where its vbPrevMatched lies.  (Owners of the ladder variants are the exception: their
descriptor is the target's plus Do private bits, see _variant.)

Two layouts:
  sites   window 5: the frame is tiled with 16-pixel sites; a group's features lie within a few pixels of its site's centre and
          nothing of another site is within any window of this one.
  line    window 110: frame-2 level-0 features on a horizontal line at unit spacing, x = 150 + p; vbPrevMatched = (40 + c, y)
          sees exactly the positions 0 .. c - 1 (|dx| < 110 is strict), in ascending x, which is the visiting order (columns
          outer; the features are created column by column in a shuffled column order and in ascending x inside a column, so the
          index order is not the visiting order)."""
import functools

import numpy as np

import grid_model as G

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
GP = G.grid_params(0, 512, 0, 384)
LINE_X0, LINE_WINDOW = 150, 110
LADDER_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def desc(bits):
    a = np.zeros(256, np.uint8)
    a[list(bits)] = 1
    return np.packbits(a)


def wdesc(w):
    """A frame-2 descriptor of weight w (bits 0 .. w - 1)."""
    assert 0 <= w <= 128
    return desc(range(w))


def tdesc(t):
    """A frame-1 descriptor of t private bits (128 .. 128 + t - 1)."""
    assert 0 <= t <= 128
    return desc(range(128, 128 + t))


class _B:
    """Collects a scene.  Frame-1 features may be given an index (at=); done() fills the free indices up to n1 with fillers."""

    def __init__(self, name, window=5, nnratio=0.9, check_ori=False):
        self.name, self.window, self.nnratio, self.check_ori = name, window, nnratio, check_ori
        self.k2, self.d2 = [], []
        self.f1s, self.placed = [], {}
        self.nsite = 0

    def site(self, n=1):
        """The centre of the next free site (n > 1: of the first of n free sites in one row)."""
        if self.nsite % 30 + n > 30:
            self.nsite += 30 - self.nsite % 30
        c = (16 + 16 * (self.nsite % 30), 16 + 16 * (self.nsite // 30))
        self.nsite += n
        assert c[1] <= 368, "out of sites"
        return c

    def f2(self, c, w, dx=0.0, dy=0.0, octave=0, angle=0.0, d=None):
        self.k2.append((c[0] + dx, c[1] + dy, octave, angle))
        self.d2.append(wdesc(w) if d is None else d)
        return len(self.k2) - 1

    def f1(self, c, t=0, dx=0.0, dy=0.0, octave=0, angle=0.0, at=None, d=None):
        """A frame-1 feature whose vbPrevMatched is c + (dx, dy).  Returns its index (known at once with at=, else a handle that
        done() turns into the index: features without at= follow each other in creation order)."""
        rec = (c[0] + dx, c[1] + dy, octave, angle, tdesc(t) if d is None else d)
        if at is not None:
            assert at not in self.placed
            self.placed[at] = rec
            return at
        self.f1s.append(rec)
        return len(self.f1s) - 1

    def done(self, ix, n1=None, filler="match", empty=(8.0, 380.0), **extra):
        """Free-order features first fill the indices that at= left free, in order; the rest up to n1 are fillers: 'match' (a site
        of its own with one candidate at distance 3), 'empty' (vbPrevMatched where no feature of frame 2 is) or a callable
        (builder, index) -> record."""
        total = max(len(self.f1s) + len(self.placed), max(self.placed, default=-1) + 1, n1 or 0)
        free = iter(self.f1s)
        recs = []
        for i in range(total):
            if i in self.placed:
                recs.append(self.placed[i])
                continue
            r = next(free, None)
            if r is None:
                if filler == "match":
                    c = self.site()
                    self.f2(c, 3)
                    r = (c[0], c[1], 0, 0.0, tdesc(0))
                elif filler == "empty":
                    r = (empty[0], empty[1], 0, 0.0, tdesc(i % 5))
                else:
                    r = filler(self, i)
            recs.append(r)
        assert next(free, None) is None, "free-order features left over: give n1"
        assert not self.placed or not self.f1s, "mixing at= with free order is not supported"
        k1 = np.zeros(len(recs), KP_DTYPE)
        k2 = np.zeros(len(self.k2), KP_DTYPE)
        prev = np.zeros((len(recs), 2), f32)
        for i, r in enumerate(recs):
            prev[i] = r[0], r[1]
            # the keypoint itself lies elsewhere: only vbPrevMatched, the octave and the angle of a frame-1 feature are read
            k1[i] = (f32(r[0]) + f32(0.5), f32(r[1]) - f32(0.25), 31, r[3], 0, r[2], -1)
        for i, r in enumerate(self.k2):
            k2[i] = (r[0], r[1], 31, r[3], 0, r[2], -1)
        for a in (k1["x"], k1["y"], k2["x"], k2["y"], prev):
            assert np.isfinite(a).all()
        d1 = np.array([r[4] for r in recs], np.uint8).reshape(-1, 32)
        d2 = np.array(self.d2, np.uint8).reshape(-1, 32)
        s = dict(name=self.name, k1=k1, d1=d1, k2=k2, d2=d2, gp=GP, prev=prev, window=self.window, nnratio=self.nnratio,
                 check_ori=self.check_ori, ix=list(ix))
        s.update(extra)
        return s


def _group(b, ws, t=0, **kw):
    """One site: a frame-1 feature with t private bits and candidates of the weights ws, created in visiting order."""
    c = b.site()
    for j, w in enumerate(ws):
        b.f2(c, w, dx=-2 + 0.5 * j, dy=0.25 * j)
    return b.f1(c, t, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# comparison edges
# ---------------------------------------------------------------------------------------------------------------------

def _owner_challenger_site(b):
    """X (weight 0) and Y (16 bits among 0..15).  A: 10 private bits -- X at 10, Y at 26: takes X.  B: bits 0..2 and 7 private
    ones -- X at 10 (the owner's distance: skipped, :444), Y at 20: takes Y, alone.  C: 6 private bits -- X at 6 (strictly better:
    displaces A, which is not matched again), Y at 22 (B holds it at 20: skipped)."""
    c = b.site()
    x = b.f2(c, 0, dx=-1)
    y = b.f2(c, 16, dx=1)
    a = b.f1(c, 10)
    bb = b.f1(c, d=desc([0, 1, 2] + list(range(128, 135))))
    cc = b.f1(c, 6)
    return (a, bb, cc), (x, y)


def _octave_sites(b):
    """Octave filters on both sides (:421-425).  (1) a frame-1 feature of octave 1 beside perfect candidates of octaves 0 and 1:
    never searched; (2) one of octave 3: neither; (3) a level-0 feature whose window holds an octave-1 candidate at distance 0, an
    octave-2 one at 1 and a level-0 one at 20: takes the level-0 one, alone in its list."""
    out = []
    c = b.site()
    b.f2(c, 0, dx=-1, octave=0)
    b.f2(c, 0, dx=1, octave=1)
    out.append(b.f1(c, 0, octave=1))
    c = b.site()
    b.f2(c, 0, octave=0)
    b.f2(c, 0, dx=1, octave=3)
    out.append(b.f1(c, 0, octave=3))
    c = b.site()
    b.f2(c, 0, dx=-1, octave=1)
    b.f2(c, 1, dx=0, octave=2)
    b.f2(c, 20, dx=1, octave=0)
    out.append(b.f1(c, 0, octave=0))
    return out


def _tie_sites(b):
    """Two candidates at the same smallest distance; the one that comes first in the visiting order has the HIGHER index in two
    of the three groups (it lies in an earlier column)."""
    out = []
    for first_dx, second_dx in ((-1.0, 1.0), (4.5, -4.5), (4.5, -4.5)):
        c = b.site()
        b.f2(c, 12, dx=first_dx)
        b.f2(c, 12, dx=second_dx)
        if len(out) == 2:
            b.f2(c, 40, dx=0.0)            # a third candidate behind the tie
        out.append(b.f1(c, 0))
    return out


def comparison_scenes():
    S = []
    b = _B("compare_0p8", nnratio=0.8)
    ix = [_group(b, ws) for ws in ([50], [51], [8, 10], [4, 5], [40, 50], [7, 10], [20], [10, 8], [50, 40], [12, 12], [12, 12, 40])]
    ix += [_group(b, [8, 10], t=2), _group(b, [5, 7], t=3)]          # 10 against 12 (12 * 0.8f > 9.6: rejected), 8 against 10 again
    (a, bb, cc), _ = _owner_challenger_site(b)
    ix += [a, bb, cc] + _octave_sites(b)
    S.append(b.done(ix))
    for name, ratio in (("tie_ratio_1p0", 1.0), ("tie_ratio_1p5", 1.5), ("tie_ratio_0p9", 0.9)):
        b = _B(name, nnratio=ratio)
        S.append(b.done(_tie_sites(b)))
    return S


# ---------------------------------------------------------------------------------------------------------------------
# rotation edges (check_ori): every match is a pair alone in its site, the angles give the bin
# ---------------------------------------------------------------------------------------------------------------------

def _pairs(b, rot, n, a2=0.0):
    """n isolated pairs with angle(1) - angle(2) = rot (float arithmetic: the angles are chosen so that it is exact)."""
    out = []
    for j in range(n):
        c = b.site()
        base = f32(a2) + f32(j % 3) * f32(16.0)
        a1 = f32(base + f32(rot))
        assert f32(a1 - base) == f32(rot) and 0 <= a1 < 360 and 0 <= base < 360
        b.f2(c, 5, angle=base)
        out.append(b.f1(c, 0, angle=a1))
    return out


def rotation_scenes():
    S = []
    # rot = 15 and 135: rot * (1.0f / 30) is exactly 0.5f and 4.5f -- round() gives bins 1 and 5, half-to-even 0 and 4
    b = _B("rot_half", check_ori=True)
    ix = _pairs(b, 15, 2) + _pairs(b, 30, 2) + _pairs(b, 0, 3) + _pairs(b, 135, 1) + _pairs(b, 150, 2) + _pairs(b, 120, 2) + \
        _pairs(b, 300, 5)
    S.append(b.done(ix))
    # rot = 14.999999f: the float product rounds up to 0.5f (bin 1), the double product stays below it (bin 0)
    b = _B("rot_below_half", check_ori=True)
    below = f32(14.999999)
    assert below < 15 and f32(below * (f32(1) / f32(30))) == f32(0.5) and float(below) * float(f32(1) / f32(30)) < 0.5
    ix = []
    for _ in range(2):                                   # (not through _pairs: angle(2) = 0 keeps the difference exact)
        c = b.site()
        b.f2(c, 5, angle=0.0)
        ix.append(b.f1(c, 0, angle=below))
    ix += _pairs(b, 30, 1) + _pairs(b, 0, 2) + _pairs(b, 150, 4) + _pairs(b, 240, 3)
    S.append(b.done(ix))
    # negative differences: 10 - 350 = -340 -> 20 (bin 1); 0 - 359.5 -> 0.5 (bin 0); -0.0 stays
    b = _B("rot_wrap", check_ori=True)
    ix = []
    for a1, a2 in ((10, 350), (10, 350), (20, 0), (5, 345), (0, 359.5), (0, 240), (0, 240), (30, 210), (0, 180), (100, 280), (0, 90)):
        c = b.site()
        b.f2(c, 5, angle=float(a2))
        ix.append(b.f1(c, 0, angle=float(a1)))
    S.append(b.done(ix))
    # ComputeThreeMaxima: 0.1f * 10.0f == 1.0f, so 1 < 1.0f fails and bins two and three stay; 0.1f * 11.0f > 1
    for name, counts in (("rot_10_1_1", (10, 1, 1)), ("rot_11_1_1", (11, 1, 1)), ("rot_20_2_1", (20, 2, 1)),
                         ("rot_1_1_10", (1, 1, 10)), ("rot_equal_bins", (2, 2, 2, 2)), ("rot_3_3_2_2", (3, 2, 3, 2, 1))):
        b = _B(name, check_ori=True)
        ix = []
        for k, n in enumerate(counts):
            ix += _pairs(b, 60 + 90 * k if len(counts) <= 4 else 30 + 60 * k, n)
        S.append(b.done(ix))
    # displaced features stay in the histogram: bins 0 / 1 / 2 / 3 hold 3 / 2 / 2 / 1 matches and bin 3 two displaced features
    # more -- with them bin 3 is a maximum and bin 2 goes, without them bin 3 goes
    b = _B("rot_displaced", check_ori=True)
    ix = []
    for _ in range(2):
        c = b.site()
        b.f2(c, 0, angle=0.0)
        ix.append(b.f1(c, 10, angle=90.0))        # accepted in bin 3, then displaced by
        ix.append(b.f1(c, 6, angle=0.0))          # this one, bin 0
    ix += _pairs(b, 0, 1) + _pairs(b, 30, 2) + _pairs(b, 60, 2) + _pairs(b, 90, 1)
    S.append(b.done(ix))
    return S


# ---------------------------------------------------------------------------------------------------------------------
# the list-length ladder
# ---------------------------------------------------------------------------------------------------------------------

def _line(b, weights, y=100.0, length=None):
    """Frame-2 level-0 features at x = 150 + p with the given weights (see the module docstring for the index order), octave-1
    features of weight 0 half a pixel beside every eighth.  Returns the feature index of every position."""
    n = len(weights) if length is None else length
    cols = {}
    for p in range(n):
        cols.setdefault(G.c_round(G.cell_coord(LINE_X0 + p, GP[0], GP[2])), []).append(p)
    order = list(cols)
    np.random.default_rng(n).shuffle(order)
    idx = {}
    for col in order:
        for p in cols[col]:
            idx[p] = b.f2((LINE_X0 + p, y), weights[p])
            if p % 8 == 3:
                b.f2((LINE_X0 + p + 0.5, y), 0, octave=1)
    return [idx[p] for p in range(n)]


def _prefix_prev(c, y=100.0):
    return (LINE_X0 - LINE_WINDOW + c, y)


def _variant(name, c, wpos, owners=(), nnratio=0.9):
    """One probe with a list of exactly c entries: the weights of wpos at their positions, 30 + p % 7 elsewhere (many ties), and
    weight 1 beyond the window (a list one entry too long would be seen).  owners = [(position, distance)]: earlier frame-1
    features that take that position at that distance."""
    b = _B("ladder/" + name, window=LINE_WINDOW, nnratio=nnratio)
    w = [wpos.get(p, 30 + p % 7) if p < c else 1 for p in range(200)]
    line = _line(b, w)
    # a position with an owner carries 8 of its w bits as a code of its own among the bits 64..127: the probe still sees w + t,
    # and the owner, whose descriptor is the target's plus Do private bits, sees every other position at Do + 8 or more
    code = {}
    for k, (p, _) in enumerate(owners):
        assert p < c and w[p] >= 8 and p not in code
        code[p] = desc(list(range(w[p] - 8)) + list(range(64 + 8 * k, 72 + 8 * k)))
        b.d2[line[p]] = code[p]
    prev = _prefix_prev(c)
    own_rows = []
    for p, do in owners:
        own_rows.append(b.f1(prev, d=code[p] | tdesc(do)))
    probe = b.f1(prev, 0)
    return b.done([probe], lad=dict(count=c, owners=[(r, line[p], do) for r, (p, do) in zip(own_rows, owners)], line=line, wpos=dict(wpos)))


def ladder_variants():
    S = []
    BEST, SECOND, FAIL = 10, 14, 11                      # 10 < 14 * 0.9f passes, 10 < 11 * 0.9f fails
    k = 0
    for c in LADDER_COUNTS[1:]:
        winners = sorted({p for p in (0, c - 1, 63, 64, 127) if p < c})
        for pw in winners:
            seconds = sorted({p for p in (pw - 1, pw + 1, (pw + c // 2) % c) if 0 <= p < c and p != pw}) or [None]
            for ps in seconds:
                k += 1
                wpos = {pw: BEST}
                if ps is not None:
                    wpos[ps] = FAIL if k % 3 == 0 else SECOND
                S.append(_variant("c%d_w%d_s%s%s" % (c, pw, ps, "_fail" if k % 3 == 0 and ps is not None else ""), c, wpos))
    # two equal minima: the first in visiting order wins the index (nnratio 1.5 lets the match through)
    for c, p1, p2 in ((2, 0, 1), (64, 0, 63), (64, 62, 63), (65, 63, 64), (65, 0, 64), (128, 63, 64), (128, 64, 127), (129, 127, 128),
                      (129, 0, 128), (200, 127, 128), (200, 64, 199)):
        S.append(_variant("c%d_tie_%d_%d" % (c, p1, p2), c, {p1: BEST, p2: BEST}, nnratio=1.5))
    # entries owned before the probe comes: the winner at a smaller, an equal (both skipped: the runner-up wins) and a larger
    # distance (displaced); the runner-up at an equal (skipped: the ratio test now passes) and a larger one (it still fails)
    for c in (2, 63, 64, 65, 127, 128, 129, 200):
        pw, ps = c - 1, (c - 1) // 2
        for tag, wpos, owners in (("win_lt", {pw: BEST, ps: SECOND}, [(pw, BEST - 2)]),
                                  ("win_eq", {pw: BEST, ps: SECOND}, [(pw, BEST)]),
                                  ("win_gt", {pw: BEST, ps: SECOND}, [(pw, BEST + 2)]),
                                  ("second_eq", {pw: BEST, ps: FAIL}, [(ps, FAIL)]),
                                  ("second_gt", {pw: BEST, ps: FAIL}, [(ps, FAIL + 2)]),
                                  ("both", {ps: BEST, pw: SECOND}, [(ps, BEST), (pw, SECOND + 3)] + ([(0, 31)] if ps > 0 else []))):
            S.append(_variant("c%d_%s" % (c, tag), c, wpos, owners))
    return S


def ladder_scene():
    """The ladder in one frame pair: two lines 160 pixels apart (further than the window), ten probes on each with exactly
    LADDER_COUNTS candidates.  Line A (y = 100): the weight at position c - 1 is the smallest of the first c for every count, so
    each probe takes the last entry of its list while the earlier winners sit in it at their owners' distance (skipped).  Line
    B (y = 260): position 0 is the best entry of every list and the probes' private bits go down from 8 to 0 -- each takes
    position 0 from the one before."""
    b = _B("ladder", window=LINE_WINDOW)
    counts = [c for c in LADDER_COUNTS if c > 0]
    wa = [48] * 200
    for c, w in zip(counts, (44, 38, 32, 27, 22, 18, 14, 11, 8)):
        wa[c - 1] = w
    wb = [10] + [30 + p % 5 for p in range(1, 200)]
    _line(b, wa, y=100.0)
    _line(b, wb, y=260.0)
    ix = []
    for y in (100.0, 260.0):
        t = 9
        for c in LADDER_COUNTS:
            if y == 260.0 and c > 0:
                t -= 1
            ix.append(b.f1(_prefix_prev(c, y), t if y == 260.0 else 0))
            b.f1(_prefix_prev(c, y), 0, octave=1 + c % 3)                 # never searched
    return b.done(ix, lad=dict(counts=list(LADDER_COUNTS) * 2))


# ---------------------------------------------------------------------------------------------------------------------
# dependencies between features of frame 1
# ---------------------------------------------------------------------------------------------------------------------

DEP_KINDS = {
    # kind: ((wX, wY, wZ), t of the earlier feature I, does dropping I change J)
    # J sees X (dx -2), Y (+2), Z (+3) at its own t = 0; I sees X alone (its vbPrevMatched lies 4 pixels to the left)
    "b_gain": ((11, 10, 40), 0, True),      # X is J's second entry: Y 10 / X 11 fails the ratio test; I takes X at 11 -> skipped, Y wins
    "b_keep": ((11, 10, 40), 2, False),     # I holds X at 13 > 11: not skipped, J still fails
    "c_gain": ((10, 11, 40), 0, True),      # X is J's first entry: X 10 / Y 11 fails; I takes X at 10 -> Y 11 / Z 40 passes
    "c_lost": ((5, 10, 11), 0, True),       # X 5 / Y 10 passes; I takes X at 5 -> Y 10 / Z 11 fails: the match is lost
    "c_displace": ((5, 10, 11), 3, False),  # I holds X at 8 > 5: J takes X from I, and ends as it does without I
}


def _dep_site(b, kind, i_at, j_at):
    (wx, wy, wz), ti, _ = DEP_KINDS[kind]
    c = b.site()
    b.f2(c, wx, dx=-2)
    b.f2(c, wy, dx=2)
    b.f2(c, wz, dx=3)
    b.f1(c, ti, dx=-4, at=i_at)
    b.f1(c, 0, at=j_at)


def _dep(kind, i_at, j_at, n1, filler="match"):
    b = _B("dep_%s_%d_%d" % (kind, i_at, j_at))
    _dep_site(b, kind, i_at, j_at)
    return b.done([i_at, j_at], n1=n1, filler=filler, dep=dict(drop=i_at, rows=[j_at], changes=DEP_KINDS[kind][2]))


def _same_target(name, ts):
    """len(ts) features want the one feature X (weight 0) at the distances ts."""
    b = _B(name)
    c = b.site()
    b.f2(c, 0)
    ix = [b.f1(c, t) for t in ts]
    return b.done(ix)


def _chain(name, lanes, n1):
    """lanes[0] takes X0 at 10.  Feature q of the chain (lanes[q + 1]) sees Xq at 10 + 2q and Xq+1 at 12 + 2q and nothing else
    (the Xs lie 4 pixels apart, its vbPrevMatched between the two): with Xq held at its own distance it takes Xq+1, which the next
    one then finds held.  Without the starter every feature takes its first entry instead."""
    b = _B(name)
    m = len(lanes) - 1
    c = b.site(3)
    for q in range(m + 1):
        b.f2(c, 10 + 2 * q, dx=4.0 * q)
    b.f1(c, 0, dx=-3.0, at=lanes[0])
    for q in range(m):
        b.f1(c, 0, dx=4.0 * q + 2.0, at=lanes[q + 1])
    return b.done(lanes, n1=n1, dep=dict(drop=lanes[0], rows=list(lanes[1:]), changes=True))


def _long_between(name, lanes, n1):
    """(e) Features with long lists between short ones, on a line of 130 (window 110): a (2 entries) takes L0 at 10; b (65
    entries, unsorted list) finds L0 held and takes L64 at 12; c (130 entries, the rescan) finds both held and takes L129 at 14; d
    (2 entries, from the other end) finds L129 held and takes L128.  Each would take its predecessor's entry without it.  The
    other features of the round see L0 alone, one bit further away than a does (the first of them holds it until a comes, the
    later ones find it held at less than their distance), or nothing."""
    b = _B(name, window=LINE_WINDOW)
    w = [40 + p % 3 for p in range(130)]
    w[0], w[64], w[128], w[129] = 10, 12, 16, 14
    _line(b, w)
    ia, ib, ic, id_ = lanes
    b.f1(_prefix_prev(2), 0, at=ia)
    b.f1(_prefix_prev(65), 0, at=ib)
    b.f1((215.0, 100.0), 0, at=ic)
    b.f1((LINE_X0 + 129 + LINE_WINDOW - 2, 100.0), 0, at=id_)

    def filler(_, i):
        p = _prefix_prev(1) if i % 2 else (20.0, 330.0)
        return (p[0], p[1], 0, 0.0, tdesc(1))
    return b.done(lanes, n1=n1, filler=filler, dep=dict(drop=ia, rows=[ib, ic, id_], changes=True),
                  lad=dict(lists={ia: 2, ib: 65, ic: 130, id_: 2}))


def dependency_scenes():
    S = []
    # (a) everybody wants X
    S.append(_same_target("same_2_decreasing", [9, 8]))
    S.append(_same_target("same_2_equal", [7, 7]))
    # TH_LOW = 50 leaves 51 acceptable distances: of 64 features at 63, 62, .. 0 the first 13 are turned away and each of the
    # other 51 takes X from the one before
    S.append(_same_target("same_64_decreasing", [63 - i for i in range(64)]))
    S.append(_same_target("same_64_equal", [7] * 64))
    S.append(_same_target("same_64_increasing", [i // 2 for i in range(64)]))
    # (b), (c): inside a round on neighbouring lanes and across the halves of the wave; between rounds
    for kind in DEP_KINDS:
        for i_at, j_at, n1 in ((0, 1, 64), (31, 32, 64), (62, 63, 64), (0, 63, 64), (63, 64, 130), (127, 128, 130)):
            S.append(_dep(kind, i_at, j_at, n1))
    # (d)
    S.append(_chain("chain_5_6_7", [5, 6, 7], 64))
    S.append(_chain("chain_0_31_32_63", [0, 31, 32, 63], 64))
    S.append(_chain("chain_62_63_64_65", [62, 63, 64, 65], 130))
    # (e)
    S.append(_long_between("long_between_3_20_40_60", [3, 20, 40, 60], 64))
    S.append(_long_between("long_between_62_63_64_65", [62, 63, 64, 65], 70))
    S.append(_long_between("long_between_126_127_128_129", [126, 127, 128, 129], 130))
    return S


def boundary_scenes():
    S = []
    for n1 in (1, 63, 64, 65, 128):
        if n1 == 1:
            b = _B("n1_1")
            _group(b, [9, 30])
            S.append(b.done([0]))
        else:
            s = _dep("b_gain", n1 - 2, n1 - 1, n1)
            s["name"] = "n1_%d" % n1
            S.append(s)
    # one feature with a candidate, everything else searches an empty place: the first round with rows, the last feature with
    # a candidate (two empty rounds before index 129)
    for k in (0, 63, 64, 129):
        b = _B("only_%d" % k)
        c = b.site()
        b.f2(c, 9)
        b.f2(c, 30, dx=1)
        b.f1(c, 0, at=k)
        S.append(b.done([k], n1=130, filler="empty"))
    return S


ROUND_BOUNDARY = "dep_b_gain_127_128"      # the scene the largest accepted caps run
CHAIN_64 = "same_64_decreasing"


@functools.lru_cache(maxsize=None)
def all_scenes():
    """Every scene, built once per process and shared; nobody changes one (tests/init_search_model.py run() keeps the window
    lists it computed under '_cands')."""
    S = comparison_scenes() + rotation_scenes() + [ladder_scene()] + ladder_variants() + dependency_scenes() + boundary_scenes()
    names = [s["name"] for s in S]
    assert len(set(names)) == len(names)
    for s in S:
        assert len(s["k1"]) <= 400 and len(s["k2"]) <= 500
    return S


def by_name(name):
    return [s for s in all_scenes() if s["name"] == name][0]
