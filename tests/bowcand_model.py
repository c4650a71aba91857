"""Model of SearchByBoW against candidate key frames (orbhip_search_by_bow_candidates): the two loops of the reference,
SearchByBoW(pKF, F, ...) (ref: src/ORBmatcher.cc:159-288) and SearchByBoW(pKF1, pKF2, ...) (:522-655), on plain Python data, with
the rotation check (:236-246, :267-285, ComputeThreeMaxima :1629-1670) and the walk of the PnPsolver constructor (ref:
src/PnPsolver.cc:78-101) with the mvMaxError loop of SetRansacParameters (:154-156).

A side is a dict: desc [n][32] uint8, angle [n] float32, x / y [n] float32, octave [n] int, fv {node: [feature indices]} (a
DBoW2::FeatureVector: iteration in ascending node id), points [n] of None or Point(bad, pos).  A frame has no points."""
import collections
import math

import numpy as np

f32 = np.float32
HISTO_LENGTH = 30
Point = collections.namedtuple("Point", "bad pos")


def distance(a, b):
    """DescriptorDistance: the number of differing bits."""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _good(p):
    return p is not None and not p.bad


def _bin(a1, a2):
    """round(rot * factor) as the reference computes it in float, rot = angle1 - angle2 (+ 360 when negative)."""
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * (f32(1.0) / f32(HISTO_LENGTH))))
    b = int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))   # C round(): halves away from zero
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ComputeThreeMaxima over the bin sizes."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1 = m2, m1, s
            i3, i2, i1 = i2, i1, i
        elif s > m2:
            m3, m2 = m2, s
            i3, i2 = i2, i
        elif s > m3:
            m3, i3 = s, i
    if f32(m2) < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif f32(m3) < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def _best_two(d1, side2, cands):
    b1, b2, bi = 256, 256, -1
    for i2 in cands:
        d = distance(d1, side2["desc"][i2])
        if d < b1:
            b2, b1, bi = b1, d, i2
        elif d < b2:
            b2 = d
    return b1, b2, bi


def _rotation(hist, clear):
    """Clears the matches of every bin but the three largest; returns how many went."""
    keep = three_maxima([len(h) for h in hist])
    gone = 0
    for i in range(HISTO_LENGTH):
        if i in keep:
            continue
        for j in hist[i]:
            clear(j)
            gone += 1
    return gone


def search_kf_frame(kf, frame, th=50, nnratio=0.75, check_ori=True):
    """SearchByBoW(pKF, F, vpMapPointMatches): returns (matches [F.N]: the key frame's feature whose point went to the frame's feature,
    or -1; nmatches)."""
    nF = len(frame["desc"])
    matches = [-1] * nF
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    for node in sorted(set(kf["fv"]) & set(frame["fv"])):
        for iKF in kf["fv"][node]:
            if not _good(kf["points"][iKF]):
                continue
            b1, b2, bi = _best_two(kf["desc"][iKF], frame, [iF for iF in frame["fv"][node] if matches[iF] < 0])
            if b1 <= th and f32(b1) < f32(nnratio) * f32(b2):
                matches[bi] = iKF
                if check_ori:
                    b = _bin(kf["angle"][iKF], frame["angle"][bi])
                    assert 0 <= b < HISTO_LENGTH
                    hist[b].append(bi)
                nm += 1
    if check_ori:
        def clear(iF):
            matches[iF] = -1
        nm -= _rotation(hist, clear)
    return matches, nm


def search_kf_kf(kf1, kf2, th=50, nnratio=0.75, check_ori=True):
    """SearchByBoW(pKF1, pKF2, vpMatches12): returns (matches12 [N1]: the feature of key frame 2, or -1; nmatches)."""
    n1, n2 = len(kf1["desc"]), len(kf2["desc"])
    m12 = [-1] * n1
    matched2 = [False] * n2
    hist = [[] for _ in range(HISTO_LENGTH)]
    nm = 0
    for node in sorted(set(kf1["fv"]) & set(kf2["fv"])):
        for i1 in kf1["fv"][node]:
            if not _good(kf1["points"][i1]):
                continue
            b1, b2, bi = _best_two(kf1["desc"][i1], kf2,
                                   [i2 for i2 in kf2["fv"][node] if not matched2[i2] and _good(kf2["points"][i2])])
            if b1 < th and f32(b1) < f32(nnratio) * f32(b2):
                m12[i1] = bi
                matched2[bi] = True
                if check_ori:
                    b = _bin(kf1["angle"][i1], kf2["angle"][bi])
                    assert 0 <= b < HISTO_LENGTH
                    hist[b].append(i1)
                nm += 1
    if check_ori:
        def clear(i1):
            m12[i1] = -1
        nm -= _rotation(hist, clear)
    return m12, nm


def pnp_setup(frame, kf, matches, level_sigma2, th2):
    """PnPsolver::PnPsolver(F, vpMapPointMatches) and mvMaxError: (mvKeyPointIndices, the key frame's features, mvP3Dw, mvP2D,
    mvMaxError) over the frame's features in ascending index."""
    kp, kfi, P3, P2, me = [], [], [], [], []
    for i, j in enumerate(matches):
        if j < 0:
            continue
        p = kf["points"][j]
        if p is None or p.bad:
            continue
        kp.append(i)
        kfi.append(j)
        P2.append((f32(frame["x"][i]), f32(frame["y"][i])))
        P3.append(tuple(f32(v) for v in p.pos))
        me.append(f32(f32(level_sigma2[frame["octave"][i]]) * f32(th2)))
    return kp, kfi, P3, P2, me


def candidates(mode, fixed, cands, th=50, nnratio=0.75, check_ori=True, gather=None):
    """The whole call.  mode 0: fixed is the frame; mode 1: fixed is the current key frame.  gather = (min_matches, level_sigma2,
    th2) or None.  Returns {"matches": [K][n_fixed], "nmatches": [K]} and, with gather, off / kp_idx / kf_idx / P3Dw / P2D /
    max_err."""
    rows, nms = [], []
    for c in cands:
        r, n = search_kf_frame(c, fixed, th, nnratio, check_ori) if mode == 0 else search_kf_kf(fixed, c, th, nnratio, check_ori)
        rows.append(r)
        nms.append(n)
    out = {"matches": rows, "nmatches": nms}
    if gather is not None:
        assert mode == 0
        min_matches, sigma2, th2 = gather
        off, kp, kfi, P3, P2, me = [0], [], [], [], [], []
        for c, r, n in zip(cands, rows, nms):
            if n >= min_matches:     # Tracking::Relocalization: nmatches < 15 discards the candidate
                a = pnp_setup(fixed, c, r, sigma2, th2)
                kp += a[0]; kfi += a[1]; P3 += a[2]; P2 += a[3]; me += a[4]
            off.append(len(kp))
        out.update(off=off, kp_idx=kp, kf_idx=kfi, P3Dw=P3, P2D=P2, max_err=me)
    return out


# ---- the same sides in the forms the other implementations take ----
def csr(fv):
    """{node: [idx]} -> (node, off, idx) arrays over ascending node ids."""
    nodes = sorted(fv)
    off, idx = [0], []
    for g in nodes:
        idx += list(fv[g])
        off.append(len(idx))
    return np.asarray(nodes, np.int32), np.asarray(off, np.int32), np.asarray(idx, np.int32)


def valid_bytes(side):
    return np.asarray([1 if _good(p) else 0 for p in side["points"]], np.uint8)
