"""Independent, definition-level Python models used to cross-check the C oracle.

They are deliberately written from the *definitions* (brute force, python lists), not from the
oracle's C code, so that an error in the oracle's optimised formulation shows up as a mismatch.
Sized for small inputs only.
"""
import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_is_corner(img, x, y, t):
    """FAST-9/16 by definition: >= 9 contiguous ring pixels all brighter than p+t or all darker
    than p-t (cv::FAST TYPE_9_16; called from src/ORBextractor.cc:811,816)."""
    v = int(img[y, x])
    q = [int(img[y + dy, x + dx]) for dx, dy in RING]
    for sign in (1, -1):
        flags = [(sign * (qq - v)) > t for qq in q]
        for s in range(16):
            if all(flags[(s + j) % 16] for j in range(9)):
                return True
    return False


def fast_score(img, x, y):
    """Score by definition: the largest t for which the pixel is still a corner (-1 if never)."""
    best = -1
    for t in range(0, 256):
        if fast_is_corner(img, x, y, t):
            best = t
        else:
            break
    return best


def fast9_16(img, th):
    """Whole cv::FAST(img, th, nonmax=True) on a small image, raster order [(x, y, score)]."""
    h, w = img.shape
    score = np.zeros((h, w), np.int32)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if fast_is_corner(img, x, y, th):
                score[y, x] = fast_score(img, x, y)
    out = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            s = score[y, x]
            if s == 0 and not fast_is_corner(img, x, y, th):
                continue
            nb = [score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx or dy)]
            if all(s > n for n in nb):
                out.append((x, y, int(s)))
    return out


def level_candidates(img, ini=20, mn=7):
    """Cell loop of ComputeKeyPointsOctTree (src/ORBextractor.cc:767-831), python ints."""
    import math
    h, w = img.shape
    minB = 16
    maxBX, maxBY = w - 16, h - 16
    width, height = np.float32(maxBX - minB), np.float32(maxBY - minB)
    nCols, nRows = int(width / np.float32(30)), int(height / np.float32(30))
    wCell = int(math.ceil(width / np.float32(nCols)))
    hCell = int(math.ceil(height / np.float32(nRows)))
    out = []
    for i in range(nRows):
        iniY = minB + i * hCell
        maxY = iniY + hCell + 6
        if iniY >= maxBY - 3:
            continue
        maxY = min(maxY, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            maxX = iniX + wCell + 6
            if iniX >= maxBX - 6:
                continue
            maxX = min(maxX, maxBX)
            sub = img[iniY:maxY, iniX:maxX]
            k = fast9_16(sub, ini)
            if not k:
                k = fast9_16(sub, mn)
            out += [(x + j * wCell, y + i * hCell, s) for x, y, s in k]
    return out


class _Node:
    __slots__ = ("ulx", "uly", "brx", "bry", "keys", "nomore", "seq")


def distribute_octtree(cands, width, height, N):
    """DistributeOctTree (src/ORBextractor.cc:541-765) with a python list as std::list.
    cands: list of (x, y, score).  Pointer tie-break -> creation sequence (later = greater).
    Returns indices into cands in result order."""
    import math
    f32 = np.float32
    nIni = int(math.floor(float(f32(width) / f32(height)) + 0.5))
    hX = f32(width) / f32(nIni)
    seq = [0]

    def new_node(ulx, uly, brx, bry):
        n = _Node()
        n.ulx, n.uly, n.brx, n.bry = ulx, uly, brx, bry
        n.keys = []
        n.nomore = False
        n.seq = seq[0]
        seq[0] += 1
        return n

    lst = []
    roots = []
    for i in range(nIni):
        n = new_node(int(hX * f32(i)), 0, int(hX * f32(i + 1)), height)
        lst.append(n)
        roots.append(n)
    for idx, (x, y, s) in enumerate(cands):
        roots[int(f32(x) / hX)].keys.append(idx)
    keep = []
    for n in lst:
        if len(n.keys) == 1:
            n.nomore = True
            keep.append(n)
        elif len(n.keys) > 1:
            keep.append(n)
    lst = keep

    def divide(n):
        halfX = int(math.ceil(float(f32(n.brx - n.ulx) / f32(2))))
        halfY = int(math.ceil(float(f32(n.bry - n.uly) / f32(2))))
        mx, my = n.ulx + halfX, n.uly + halfY
        ch = [new_node(n.ulx, n.uly, mx, my), new_node(mx, n.uly, n.brx, my),
              new_node(n.ulx, my, mx, n.bry), new_node(mx, my, n.brx, n.bry)]
        for idx in n.keys:
            x, y, _ = cands[idx]
            if x < mx:
                k = 0 if y < my else 2
            else:
                k = 1 if y < my else 3
            ch[k].keys.append(idx)
        for c in ch:
            if len(c.keys) == 1:
                c.nomore = True
        return ch

    finish = False
    while not finish:
        prev_size = len(lst)
        n_to_expand = 0
        vsz = []
        i = 0
        # iterate front->back over the nodes present at the start of the pass
        snapshot = list(lst)
        for n in snapshot:
            if n.nomore:
                continue
            for c in divide(n):
                if c.keys:
                    lst.insert(0, c)
                    if len(c.keys) > 1:
                        n_to_expand += 1
                        vsz.append(c)
            lst.remove(n)
        if len(lst) >= N or len(lst) == prev_size:
            finish = True
        elif len(lst) + n_to_expand * 3 > N:
            while not finish:
                prev_size = len(lst)
                prev = sorted(vsz, key=lambda c: (len(c.keys), c.seq))
                vsz = []
                for n in reversed(prev):
                    for c in divide(n):
                        if c.keys:
                            lst.insert(0, c)
                            if len(c.keys) > 1:
                                vsz.append(c)
                    lst.remove(n)
                    if len(lst) >= N:
                        break
                if len(lst) >= N or len(lst) == prev_size:
                    finish = True
    out = []
    for n in lst:
        best = n.keys[0]
        for k in n.keys[1:]:
            if cands[k][2] > cands[best][2]:
                best = k
        out.append(best)
    return out


def hamming(a, b):
    return sum(int(x ^ y).bit_count() for x, y in zip(bytes(a), bytes(b)))


def search_by_bow(desc1, valid1, angle1, fv1, desc2, valid2, angle2, fv2, th, strict, ratio,
                  check_ori):
    """SearchByBoW (src/ORBmatcher.cc:159-288 / :522-655) on dict FeatureVectors
    {node: [feature indices]} (std::map iteration = ascending node id)."""
    n1, n2 = len(desc1), len(desc2)
    m12 = [-1] * n1
    m21 = [-1] * n2
    hist = [[] for _ in range(30)]
    nm = 0
    for node in sorted(set(fv1) & set(fv2)):
        for i1 in fv1[node]:
            if not valid1[i1]:
                continue
            b1, b2, bi = 256, 256, -1
            for i2 in fv2[node]:
                if m21[i2] >= 0:
                    continue
                if valid2 is not None and not valid2[i2]:
                    continue
                d = hamming(desc1[i1], desc2[i2])
                if d < b1:
                    b2, b1, bi = b1, d, i2
                elif d < b2:
                    b2 = d
            ok = (b1 < th) if strict else (b1 <= th)
            if ok and np.float32(b1) < np.float32(ratio) * np.float32(b2):
                m12[i1] = bi
                m21[bi] = i1
                if check_ori:
                    rot = np.float32(angle1[i1]) - np.float32(angle2[bi])
                    if rot < 0:
                        rot = np.float32(rot + np.float32(360.0))
                    v = float(np.float32(rot * (np.float32(1.0) / np.float32(30))))
                    import math
                    b = int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))
                    if b == 30:
                        b = 0
                    hist[b].append(i1)
                nm += 1
    if check_ori:
        sizes = [len(h) for h in hist]
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
        if np.float32(m2) < np.float32(0.1) * np.float32(m1):
            i2 = i3 = -1
        elif np.float32(m3) < np.float32(0.1) * np.float32(m1):
            i3 = -1
        for i in range(30):
            if i in (i1, i2, i3):
                continue
            for a in hist[i]:
                m21[m12[a]] = -1
                m12[a] = -1
                nm -= 1
    return nm, m12, m21


# ---- Frame::ComputeStereoMatches (src/Frame.cc:810-984), restated from the reference ----
STEREO_BRANCHES = ("band_empty", "octave_rejected", "no_candidate_under_75", "border_skip", "bestinc_at_edge",
                   "deltaR_out", "disparity_out", "disparity_zero", "median_cut", "kept", "median_above_255")

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _roundf(v):
    """C++ round(float): halves away from zero (np.round would round them to even)."""
    v = np.float32(v)
    r = np.floor(np.abs(v))
    if np.abs(v) - r >= np.float32(0.5):
        r += np.float32(1)
    return np.float32(np.copysign(r, v))


def stereo_matches(pyrL, pyrR, kL, dL, kR, dR, scale_factors, inv_scale_factors, mb, mbf):
    """pyrL / pyrR: lists of pyramid levels (uint8 2-D); kL / kR: keypoint records (x, y, octave); dL / dR: [n, 32] uint8.
    float32 throughout, in the reference's operation order.  Returns (mvuRight, mvDepth, n_before_cut, counters): one
    outcome counter per left keypoint (band_empty / no_candidate_under_75 / border_skip / bestinc_at_edge / deltaR_out /
    disparity_out / median_cut / kept), plus disparity_zero (accepted with disparity == 0), octave_rejected (candidate pairs
    dropped by the +-1 octave rule) and median_above_255 (1 when the median patch distance exceeds one byte).
    Where the reference is undefined (a band row outside the image, an empty match set) the model does what the oracle
    documents; a patch read outside the image raises instead of wrapping around."""
    f32 = np.float32
    cnt = dict.fromkeys(STEREO_BRANCHES, 0)
    sf = [f32(s) for s in scale_factors]
    isf = [f32(s) for s in inv_scale_factors]
    nL, nR = len(kL), len(kR)
    uRight = np.full(nL, -1.0, np.float32)
    depth = np.full(nL, -1.0, np.float32)
    nRows = pyrL[0].shape[0]
    rows = [[] for _ in range(nRows)]                          # vRowIndices, :822-836 (ascending iR in every row)
    for iR in range(nR):
        kpY = f32(kR["y"][iR])
        r = f32(2.0) * sf[int(kR["octave"][iR])]
        maxr, minr = int(np.ceil(kpY + r)), int(np.floor(kpY - r))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:
                rows[yi].append(iR)
    minZ = f32(mb)
    minD = f32(0)
    maxD = f32(mbf) / minZ
    xR = kR["x"].astype(np.float32)
    octR = kR["octave"].astype(np.int64)
    dR = np.asarray(dR, np.uint8).reshape(-1, 32)
    dL = np.asarray(dL, np.uint8).reshape(-1, 32)
    vDistIdx = []
    w = L = 5
    for iL in range(nL):
        levelL = int(kL["octave"][iL])
        vL, uL = f32(kL["y"][iL]), f32(kL["x"][iL])
        row = int(vL)                                          # vRowIndices[vL]: float -> size_t truncates
        cand = rows[row] if 0 <= row < nRows else []
        if not cand:
            cnt["band_empty"] += 1
            continue
        minU, maxU = uL - maxD, uL - minD
        if maxU < 0:
            cnt["band_empty"] += 1
            continue
        cand = np.array(cand, np.int64)
        octok = (octR[cand] >= levelL - 1) & (octR[cand] <= levelL + 1)
        cnt["octave_rejected"] += int((~octok).sum())
        cand = cand[octok]
        cand = cand[(xR[cand] >= minU) & (xR[cand] <= maxU)]
        bestDist, bestIdxR = 100, 0                            # TH_HIGH
        if len(cand):
            dist = _POP8[dL[iL][None, :] ^ dR[cand]].sum(axis=1)
            j = int(np.argmin(dist))                           # first minimum in ascending iR = the strict '<' scan
            if dist[j] < bestDist:
                bestDist, bestIdxR = int(dist[j]), int(cand[j])
        if not bestDist < (100 + 50) // 2:
            cnt["no_candidate_under_75"] += 1
            continue
        uR0 = xR[bestIdxR]
        scaleFactor = isf[levelL]
        scaleduL = _roundf(uL * scaleFactor)
        scaledvL = _roundf(vL * scaleFactor)
        scaleduR0 = _roundf(uR0 * scaleFactor)
        imL, imR = pyrL[levelL], pyrR[levelL]
        iniu = scaleduR0 + f32(L - w)
        endu = scaleduR0 + f32(L + w + 1)
        if iniu < 0 or endu >= imR.shape[1]:
            cnt["border_skip"] += 1
            continue
        cy, cxL, cxR = int(scaledvL), int(scaleduL), int(scaleduR0)
        if not (cy - w >= 0 and cy + w < imL.shape[0] and cxL - w >= 0 and cxL + w < imL.shape[1] and cxR - L - w >= 0
                and cxR + L + w < imR.shape[1]):
            raise ValueError("stereo model: the patches of left keypoint %d leave the image (undefined in the reference)" % iL)
        IL = imL[cy - w:cy + w + 1, cxL - w:cxL + w + 1].astype(np.float32)
        IL = IL - IL[w, w]
        bestSad, bestincR = 2147483647, 0
        vDists = np.zeros(2 * L + 1, np.float32)
        for incR in range(-L, L + 1):
            IR = imR[cy - w:cy + w + 1, cxR + incR - w:cxR + incR + w + 1].astype(np.float32)
            IR = IR - IR[w, w]
            d = f32(np.abs(IL.astype(np.float64) - IR).sum())  # cv::norm(NORM_L1) in double, stored in a float
            if d < f32(bestSad):
                bestSad = int(d)
                bestincR = incR
            vDists[L + incR] = d
        if bestincR == -L or bestincR == L:
            cnt["bestinc_at_edge"] += 1
            continue
        dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = (dist1 - dist3) / (f32(2.0) * (dist1 + dist3 - f32(2.0) * dist2))
        if deltaR < -1 or deltaR > 1:
            cnt["deltaR_out"] += 1
            continue
        bestuR = sf[levelL] * (f32(scaleduR0) + f32(bestincR) + deltaR)
        disparity = uL - bestuR
        if disparity >= minD and disparity < maxD:
            if disparity <= 0:
                cnt["disparity_zero"] += 1
                disparity = f32(0.01)
                bestuR = f32(np.float64(uL) - 0.01)            # `uL-0.01` is a double expression, :957
            depth[iL] = f32(mbf) / disparity
            uRight[iL] = bestuR
            vDistIdx.append((bestSad, iL))
        else:
            cnt["disparity_out"] += 1
    n = len(vDistIdx)
    if n:
        vDistIdx.sort()
        median = f32(vDistIdx[n // 2][0])
        thDist = f32(1.5) * f32(1.4) * median
        cnt["median_above_255"] += int(vDistIdx[n // 2][0] > 255)
        for i in range(n - 1, -1, -1):
            if f32(vDistIdx[i][0]) < thDist:
                break
            uRight[vDistIdx[i][1]] = -1
            depth[vDistIdx[i][1]] = -1
            cnt["median_cut"] += 1
    cnt["kept"] = n - cnt["median_cut"]
    return uRight, depth, n, cnt
