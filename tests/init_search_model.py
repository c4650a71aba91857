"""ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520) and ComputeThreeMaxima (:1629-1670) at definition level:
no device, no liborbhip, no oracle.  The windows come from tests/grid_model.py (grid_build, features_in_area); every float
operation is one np.float32 operation, as the reference's float variables make it.

search() returns the results and a trace per feature of frame 1, which tests/test_init_search_model.py uses to show that the
scenes of tests/init_search_scenes.py contain what they claim.  The `defect` argument computes what a wrong implementation
would (the guard-scene convention of tests/grid_model.py): each name of DEFECTS changes one decision, and the CPU test asserts
that every one of them changes the result of at least one scene."""
import math

import numpy as np

import grid_model as G

f32 = np.float32
INT_MAX = 2**31 - 1
TH_LOW = 50
HISTO_LENGTH = 30

DEFECTS = ("md_lt", "th_lt", "ratio_le", "ratio_double", "last_of_equal", "second_distinct", "hist_survivors", "maxima_ge",
           "tenth_le", "tenth_double", "bin_rint", "bin_double", "no_wrap", "level_any", "octave1_searches")

TRACE_DTYPE = np.dtype([("searched", "?"),       # the feature passed the octave test of :422
                        ("ncand", "<i4"),        # size of vIndices2
                        ("pos", "<i4"),          # position of bestIdx2 in the visiting order, -1 without one
                        ("best", "<i8"), ("best2", "<i8"), ("best_idx", "<i4"),
                        ("second_pos", "<i4"),   # position of the entry that gave bestDist2 its final value, -1 without one
                        ("decided", "U8"),       # 'none' (no candidate left), 'th_low' (:459 rejects), 'ratio' (:461 rejects), 'accept'
                        ("displaced", "<i4"),    # the owner that lost bestIdx2, -1 without one
                        ("bin", "<i4"),          # the rotation histogram's bin, -1 when not accepted or not checked
                        ("skip_lt", "<i4"),      # candidates skipped at :444 with vMatchedDistance < dist
                        ("skip_eq", "<i4"),      # ... with vMatchedDistance == dist
                        ("owned_gt", "<i4")])    # candidates with an owner at a larger distance (not skipped)


def three_maxima(h, defect=None):
    """ComputeThreeMaxima over the bin sizes h: (ind1, ind2, ind3)."""
    gt = (lambda a, b: a >= b) if defect == "maxima_ge" else (lambda a, b: a > b)
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(h):
        if gt(s, m1):
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif gt(s, m2):
            m3, m2, i3, i2 = m2, s, i2, i
        elif gt(s, m3):
            m3, i3 = s, i
    if defect == "tenth_double":
        tenth = float(f32(0.1)) * float(m1)
    else:
        tenth = float(f32(0.1) * f32(m1))                      # 0.1f * (float)max1, one float product (:1661)
    lt = (lambda a, b: a <= b) if defect == "tenth_le" else (lambda a, b: a < b)
    if lt(float(m2), tenth):
        i2 = i3 = -1
    elif lt(float(m3), tenth):
        i3 = -1
    return i1, i2, i3


def rotation_bin(a1, a2, defect=None):
    """The bin of :475-480 for the angles of the two matched keypoints."""
    rot = f32(a1) - f32(a2)
    if rot < 0 and defect != "no_wrap":
        rot = f32(rot + f32(360.0))
    factor = f32(1.0) / f32(HISTO_LENGTH)
    v = float(rot) * float(factor) if defect == "bin_double" else float(f32(rot * factor))
    if defect == "bin_rint":
        b = int(np.rint(v))
    else:
        b = int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)       # C round(): half away from zero
    return 0 if b == HISTO_LENGTH else b


def hamming_table(d1, d2):
    """[len(d1), len(d2)] Hamming distances of 32-byte descriptors."""
    b1 = np.unpackbits(np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    b2 = np.unpackbits(np.ascontiguousarray(d2, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    return b1 @ (1 - b2).T + (1 - b1) @ b2.T


def search(k1, d1, k2, d2, gp, prev, window, nnratio, check_ori, defect=None, cands=None):
    """The routine as the reference writes it.  Returns (nmatches, vnMatches12, vbPrevMatched after :515-517, trace).
    cands: an optional dict the caller keeps per scene; the window lists (which no defect but the two octave ones changes) are
    stored in it and taken from it."""
    assert defect is None or defect in DEFECTS
    prev = np.array(prev, f32).reshape(-1, 2)
    n1, n2 = len(k1), len(k2)
    grid = None
    dist = hamming_table(d1, d2) if n1 and n2 else np.zeros((n1, n2), np.int32)
    m12 = np.full(n1, -1, np.int64)
    m21 = np.full(n2, -1, np.int64)
    md = np.full(n2, INT_MAX, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    trace = np.zeros(n1, TRACE_DTYPE)
    for name in ("pos", "best_idx", "second_pos", "displaced", "bin"):
        trace[name] = -1
    trace["best"] = trace["best2"] = INT_MAX
    trace["decided"] = "none"
    ratio = f32(nnratio)
    n = 0
    for i1 in range(n1):
        level1 = int(k1["octave"][i1])
        if level1 > (1 if defect == "octave1_searches" else 0):                      # :421-423
            continue
        lv = (-1, -1) if defect == "level_any" else (level1, level1)
        key = (i1, lv)
        if cands is not None and key in cands:
            cand = cands[key]
        else:
            if grid is None:
                grid = G.grid_build(k2, gp)
            cand = G.features_in_area(k2, grid, gp, prev[i1, 0], prev[i1, 1], f32(window), lv[0], lv[1])   # :425
            if cands is not None:
                cands[key] = cand
        t = trace[i1]
        t["searched"], t["ncand"] = True, len(cand)
        if not cand:                                                                   # :427
            continue
        best, best2, bi, pos, pos2 = INT_MAX, INT_MAX, -1, -1, -1
        for p, i2 in enumerate(cand):
            d = int(dist[i1, i2])
            if md[i2] < INT_MAX:
                if md[i2] < d:
                    t["skip_lt"] += 1
                elif md[i2] == d:
                    t["skip_eq"] += 1
                else:
                    t["owned_gt"] += 1
            if (md[i2] < d) if defect == "md_lt" else (md[i2] <= d):                  # :444
                continue
            if (d <= best) if defect == "last_of_equal" else (d < best):              # :447
                best2, pos2 = best, pos
                best, bi, pos = d, int(i2), p
            elif d < best2 and not (defect == "second_distinct" and d == best):       # :453
                best2, pos2 = d, p
        t["best"], t["best2"], t["best_idx"], t["pos"], t["second_pos"] = best, best2, bi, pos, pos2
        if bi < 0:
            continue
        if not ((best < TH_LOW) if defect == "th_lt" else (best <= TH_LOW)):          # :459
            t["decided"] = "th_low"
            continue
        if defect == "ratio_double":
            ok = float(best) < float(f32(best2)) * float(ratio)
        elif defect == "ratio_le":
            ok = bool(f32(best) <= f32(best2) * ratio)
        else:
            ok = bool(f32(best) < f32(best2) * ratio)                                  # :461, (float)bestDist2 * mfNNratio
        if not ok:
            t["decided"] = "ratio"
            continue
        t["decided"] = "accept"
        if m21[bi] >= 0:                                                              # :463-467
            t["displaced"] = m21[bi]
            m12[m21[bi]] = -1
            n -= 1
        m12[i1], m21[bi], md[bi] = bi, i1, best
        n += 1
        if check_ori:                                                                 # :473-483
            b = rotation_bin(k1["angle"][i1], k2["angle"][bi], defect)
            t["bin"] = b
            if 0 <= b < HISTO_LENGTH:                                                 # (the reference asserts it)
                hist[b].append(i1)
    if check_ori:                                                                     # :489-512
        if defect == "hist_survivors":
            hist = [[i for i in h if m12[i] >= 0] for h in hist]
        keep = three_maxima([len(x) for x in hist], defect)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    n -= 1
    out = prev.copy()
    for i1 in np.nonzero(m12 >= 0)[0]:                                                # :515-517
        out[i1] = (k2["x"][m12[i1]], k2["y"][m12[i1]])
    return n, m12.astype(np.int32), out, trace


def run(s, defect=None, drop=None):
    """search() on a scene of tests/init_search_scenes.py.  drop: an index of frame 1 that is taken out of the walk (its octave
    becomes 1: it stays in its place and is never searched), for the dependency checks."""
    k1 = s["k1"]
    cands = s.setdefault("_cands", {})
    if drop is not None:
        k1 = k1.copy()
        k1["octave"][drop] = 1 if defect != "octave1_searches" else 2
    return search(k1, s["d1"], s["k2"], s["d2"], s["gp"], s["prev"], s["window"], s["nnratio"], s["check_ori"], defect, cands)


# ---- the LDS layout of k_init_assign (csrc/k_guided.hip:1396-1427 and the check of csrc/api_guided.hip:238) ---------------------

INIT_K = 128                              # candidate slots per feature
ROUND_BYTES = 64 * INIT_K * 4             # one round's 64 lists
LDS_BUDGET, TABLE_LIMIT = 144 * 1024, 112 * 1024
MODE_STAGED, MODE_DBL = 1, 2
# the caps the device tests allocate at: one pair per layout
CAP_PAIRS = ((2048, 2000), (2865, 2800), (4096, 4000), (5000, 5200))


def assign_tables(cap1, cap2):
    """init_assign_lds (:1396): vnMatches12 and the accepted feature [cap1 each]; vMatchedDistance, vnMatches21 and the stamps
    [cap2 each]."""
    return (2 * cap1 + 3 * cap2) * 4


def assign_mode(cap1, cap2):
    """(mode, dynamic LDS bytes) as launch_search_for_initialization chooses them (:1422-1427), or None when the API turns the
    caps away (the required tables exceed 112 KB)."""
    tables = assign_tables(cap1, cap2)
    if tables > TABLE_LIMIT:
        return None
    cap1pad = (cap1 + 63) // 64 * 64
    staged = tables + (cap1pad + cap1 + 3 * cap2) * 4          # list lengths, angles of frame 1, x / y / angle of frame 2 (:1398-1402)
    mode = MODE_STAGED if ROUND_BYTES + staged <= LDS_BUDGET else 0
    if mode:
        tables = staged
    if 2 * ROUND_BYTES + tables <= LDS_BUDGET:
        mode |= MODE_DBL
    return mode, (2 if mode & MODE_DBL else 1) * ROUND_BYTES + tables
