"""Edge scenes for the batched SearchByBoW (k_bow_lane / k_bow_seq, csrc/k_bowseq.hip; ref src/ORBmatcher.cc:159-288, :522-655),
with no device code: a descriptor builder that realises a wanted distance table, the scenes, a reach model of what the launcher
and steps 2 / 3 of k_bow_lane decide, and the definition-level model with its deliberately wrong variants.

Descriptors.  Inside a node, rows (side 1) and candidates (side 2) are grouped into components: a component is a set of rows with
identical descriptors and the candidates that are NEAR them.  Component k sits on word k of a 512-word code of 256 bits
(Sylvester-Hadamard rows and their complements: any two words differ in 128 or 256 bits); its rows are the word itself and a
near candidate at distance d is the word with d chosen bits flipped, so d(row, candidate) = d exactly and everything across
components lies at 128 +- a small imbalance.  Candidates no row is near to are fillers on a word of their own.  The builder
checks the realised table with numpy.unpackbits: near entries exact, every other entry >= FAR; it raises when it cannot.

tests/test_bowseq_edges_model.py validates all this on the CPU; tests/test_bowseq_edges_gpu.py runs the scenes on the device."""
import numpy as np

import pymodels

f32 = np.float32
TH = 50                 # orbhip_search_by_bow_seq_device passes TH_LOW
FAR = 100               # every entry of a distance table that is not planted is at least this
BL_TILES, BL_MAXN2 = 640, 128
LANE_LDS_LIMIT = 150 * 1024

_I = np.arange(256)
_PAR = np.array([bin(v).count("1") & 1 for v in range(256)], np.uint8)


def codeword(k):
    """word k of the code: row k & 255 of the Sylvester-Hadamard matrix of order 256 as bits, complemented for k >= 256"""
    return (_PAR[_I & (k & 255)] ^ (k >> 8)).astype(np.uint8)


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1, 256), axis=1, bitorder="little")


def table(desc1, desc2):
    """Hamming distances [n1, n2] of packed descriptors"""
    a = np.unpackbits(np.asarray(desc1, np.uint8).reshape(-1, 1, 32), axis=2)
    b = np.unpackbits(np.asarray(desc2, np.uint8).reshape(1, -1, 32), axis=2)
    return (a ^ b).sum(axis=2, dtype=np.int32)


def build_node(rng, comps, n2):
    """comps: [(nrows, {candidate position: distance})]; a position belongs to at most one component.  Returns (rows [n1, 256] bits,
    cands [n2, 256] bits, want [n1, n2] with -1 = 'at least FAR')."""
    assert len(comps) < 511, "more components than code words"
    owner = {}
    for k, (_, near) in enumerate(comps):
        for c, d in near.items():
            assert 0 <= c < n2 and 0 <= d <= 256 and c not in owner, "bad near entry (%d, %d)" % (c, d)
            owner[c] = k
    n1 = sum(nr for nr, _ in comps)
    want = np.full((n1, n2), -1, np.int32)
    for attempt in range(40):
        base = rng.integers(0, 2, 256).astype(np.uint8)
        words = rng.permutation(512)[:len(comps) + 1]
        rows = np.zeros((n1, 256), np.uint8)
        cands = np.zeros((n2, 256), np.uint8)
        r = 0
        for k, (nr, near) in enumerate(comps):
            w = codeword(int(words[k]))
            rows[r:r + nr] = w ^ base
            for c, d in near.items():
                m = np.zeros(256, np.uint8)
                m[rng.permutation(256)[:d]] = 1
                cands[c] = w ^ m ^ base
                want[r:r + nr, c] = d
            r += nr
        wf = codeword(int(words[len(comps)]))
        for c in range(n2):
            if c not in owner:
                m = np.zeros(256, np.uint8)
                m[rng.permutation(256)[:int(rng.integers(0, 12))]] = 1
                cands[c] = wf ^ m ^ base
        if n1 == 0 or n2 == 0:
            return rows, cands, want
        got = table(pack(rows), pack(cands))
        if ((want >= 0) & (got != want)).any():
            raise AssertionError("near entries not realised")        # cannot happen: a construction error
        if (got[want < 0] >= FAR).all():
            return rows, cands, want
    raise AssertionError("distance table not realisable: a far entry below %d in 40 draws" % FAR)


class Pair:
    """One frame pair under construction: nodes are added with their tables, then the features of each side are interleaved across
    nodes (ascending order inside a node kept: that is the FeatureVector's)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.f = ([], [])            # per side: (sort key, node id, bits, weight, valid, angle, tag)
        self.nodes = []              # (node id, want table) for the realised-table check
        self.contents = {}

    def node(self, nid, comps, n2, w1=None, w2=None, v1=None, v2=None, a1=None, a2=None, tag1=None, content=None):
        """content: nodes given the same key share one realisation of the same table"""
        if content is not None and content in self.contents:
            rows, cands, want = self.contents[content]
        else:
            rows, cands, want = build_node(self.rng, comps, n2)
            if content is not None:
                self.contents[content] = (rows, cands, want)
        for side, bits in ((0, rows), (1, cands)):
            n = len(bits)
            keys = np.sort(self.rng.random(n))
            w, v, a = (w1, v1, a1) if side == 0 else (w2, v2, a2)
            for i in range(n):
                self.f[side].append((keys[i], nid, bits[i], 1.0 if w is None else w[i], 1 if v is None else v[i],
                                     0.0 if a is None else a[i], (tag1[i] if tag1 is not None else None) if side == 0 else None))
        self.nodes.append((nid, want))

    def sides(self, shuffle=True):
        out = []
        for side in (0, 1):
            fs = sorted(self.f[side], key=lambda t: t[0]) if shuffle else self.f[side]
            n = len(fs)
            out.append({"desc": pack([t[2] for t in fs]) if n else np.zeros((0, 32), np.uint8),
                        "node": np.array([t[1] for t in fs], np.int64).astype(np.int32), "wt": np.array([t[3] for t in fs], f32),
                        "valid": np.array([t[4] for t in fs], np.uint8), "angle": np.array([t[5] for t in fs], f32),
                        "tag": [t[6] for t in fs]})
        return out


def scene(name, family, pair, cap, th_mode=0, nnratio=0.7, check_ori=1, use_valid=False, target=None, shuffle=True):
    s1, s2 = pair.sides(shuffle)
    assert len(s1["desc"]) <= cap and len(s2["desc"]) <= cap, name
    return {"name": name, "family": family, "f1": s1, "f2": s2, "cap": cap, "th_mode": th_mode, "nnratio": float(f32(nnratio)),
            "check_ori": check_ori, "use_valid": use_valid, "target": target or {}, "nodes": pair.nodes}


# --------------------------------------------------------------------------------------------------------------------------------
# the model and its wrong variants
# --------------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("second_skips_own_lane", "second_skips_own_lane64", "claimed_is_candidate", "claimed_reads_255", "dist_clamped_255",
            "le_for_lt", "lt_for_le", "ratio_in_double", "tie_takes_highest", "valid2_in_mode0", "stopped_kept", "nan_weight_kept",
            "node_ids_truncated", "adjacent_ids_merged", "maxima_ge", "cut_in_double", "round_half_even")


def fv_dict(node, wt, variant=None):
    """{node id: [feature indices ascending]} of the features with weight > 0 (IEEE: a denormal is in, NaN and -0.0 are out)"""
    wt = np.asarray(wt, f32)
    with np.errstate(invalid="ignore"):
        keep = wt > 0
        if variant == "stopped_kept":
            keep = np.ones(len(wt), bool)
        elif variant == "nan_weight_kept":
            keep = ~(wt <= 0)
    out = {}
    for i in np.nonzero(keep)[0]:
        nid = int(node[i])
        if variant == "node_ids_truncated":
            nid &= 0x3FFFFFFF
        elif variant == "adjacent_ids_merged":
            nid >>= 1
        out.setdefault(nid, []).append(int(i))
    return out


def _rot_bin(a1, a2, half_even=False):
    rot = f32(a1) - f32(a2)
    if rot < 0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * (f32(1.0) / f32(30))))
    if half_even:
        b = int(np.round(v))
    else:
        b = int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))
    return 0 if b == 30 else b


def _variant_model(f1, f2, th_mode, nnratio, check_ori, use_valid, v):
    """SearchByBoW restated with one switchable defect (v = None: no defect; the CPU test holds that form against pymodels)."""
    d1, d2 = f1["desc"], f2["desc"]
    n1, n2 = len(d1), len(d2)
    valid1 = f1["valid"] if use_valid else np.ones(n1, np.uint8)
    valid2 = f2["valid"] if (use_valid and (th_mode or v == "valid2_in_mode0")) else None
    fv1, fv2 = fv_dict(f1["node"], f1["wt"], v), fv_dict(f2["node"], f2["wt"], v)
    strict = bool(th_mode)
    if v == "le_for_lt":
        strict = False
    if v == "lt_for_le":
        strict = True
    m12, m21 = [-1] * n1, [-1] * n2
    r32 = f32(nnratio)
    for nid in sorted(set(fv1) & set(fv2)):
        l1, l2 = fv1[nid], fv2[nid]
        D = table(d1[l1], d2[l2])
        if v == "dist_clamped_255":
            D = np.minimum(D, 255)
        claimed = [False] * len(l2)
        for r, i1 in enumerate(l1):
            if not valid1[i1]:
                continue
            b1, b2, bp = 256, 256, -1
            stride = 16 if v == "second_skips_own_lane" else 64 if v == "second_skips_own_lane64" else 0
            lane_best = {}
            saw_claimed = False
            for p, i2 in enumerate(l2):
                d = int(D[r, p])
                if claimed[p]:
                    if v == "claimed_reads_255":
                        saw_claimed = True
                    if v != "claimed_is_candidate":
                        continue
                if valid2 is not None and not valid2[i2]:
                    continue
                if stride:
                    ln = p % stride
                    if ln not in lane_best or d < lane_best[ln][0]:
                        lane_best[ln] = (d, p)
                if d < b1 or (v == "tie_takes_highest" and d == b1):
                    b2, b1, bp = b1, d, p
                elif d < b2:
                    b2 = d
            if stride and bp >= 0:
                b2 = min([256] + [d for ln, (d, p) in lane_best.items() if ln != bp % stride])
            if saw_claimed:
                b2 = min(b2, 255)
            ok = (b1 < TH) if strict else (b1 <= TH)
            if v == "ratio_in_double":
                rt = float(b1) < float(r32) * float(b2)
            else:
                rt = bool(f32(b1) < r32 * f32(b2))
            if ok and rt:
                m12[i1] = l2[bp]
                m21[l2[bp]] = i1
                claimed[bp] = True
    if v == "claimed_is_candidate":         # a candidate matched twice keeps its last row, as the output pass would
        for i1 in range(n1):
            if m12[i1] >= 0 and m21[m12[i1]] != i1:
                m12[i1] = -1
    if check_ori:
        hist = [[] for _ in range(30)]
        for i1 in range(n1):
            if m12[i1] >= 0:
                hist[_rot_bin(f1["angle"][i1], f2["angle"][m12[i1]], v == "round_half_even")].append(i1)
        mx, ix = [0, 0, 0], [-1, -1, -1]
        gt = (lambda a, b: a >= b) if v == "maxima_ge" else (lambda a, b: a > b)
        for i, h in enumerate(hist):
            s = len(h)
            if gt(s, mx[0]):
                mx, ix = [s, mx[0], mx[1]], [i, ix[0], ix[1]]
            elif gt(s, mx[1]):
                mx, ix = [mx[0], s, mx[1]], [ix[0], i, ix[1]]
            elif gt(s, mx[2]):
                mx[2], ix[2] = s, i
        cut = (lambda m: float(m) < float(f32(0.1)) * float(mx[0])) if v == "cut_in_double" else (lambda m: bool(f32(m) < f32(0.1) * f32(mx[0])))
        if cut(mx[1]):
            ix[1] = ix[2] = -1
        elif cut(mx[2]):
            ix[2] = -1
        for i in range(30):
            if i not in ix:
                for a in hist[i]:
                    m21[m12[a]] = -1
                    m12[a] = -1
    return sum(1 for x in m12 if x >= 0), m12, m21


def model_pair(f1, f2, th_mode, nnratio, check_ori, use_valid, variant=None, restated=False):
    if variant is not None or restated:
        return _variant_model(f1, f2, th_mode, nnratio, check_ori, use_valid, variant)
    n1, n2 = len(f1["desc"]), len(f2["desc"])
    valid1 = f1["valid"] if use_valid else np.ones(n1, np.uint8)
    valid2 = f2["valid"] if (use_valid and th_mode) else None
    return pymodels.search_by_bow(f1["desc"], valid1, f1["angle"], fv_dict(f1["node"], f1["wt"]), f2["desc"], valid2, f2["angle"],
                                  fv_dict(f2["node"], f2["wt"]), TH, bool(th_mode), f32(nnratio), bool(check_ori))


_model_cache = {}


def model(sc, variant=None):
    """tests/pymodels.py:search_by_bow on the scene's pair; with a variant, the restated form with that defect (kept per scene)"""
    key = (sc["name"], variant)
    if key not in _model_cache:
        _model_cache[key] = _model_uncached(sc, variant)
    return _model_cache[key]


def _model_uncached(sc, variant):
    return model_pair(sc["f1"], sc["f2"], sc["th_mode"], sc["nnratio"], sc["check_ori"], sc["use_valid"], variant)


def oracle_pair(oracle, f1, f2, th_mode, nnratio, check_ori, use_valid):
    n1, n2 = len(f1["desc"]), len(f2["desc"])
    v1 = f1["valid"] if use_valid else np.ones(n1, np.uint8)
    v2 = f2["valid"] if (use_valid and th_mode) else None
    g1, g2 = oracle.feature_vector(f1["node"], f1["wt"]), oracle.feature_vector(f2["node"], f2["wt"])
    return oracle.search_by_bow(f1["desc"], v1, f1["angle"], g1, f2["desc"], v2, f2["angle"], g2, th=TH, th_mode=th_mode,
                                nnratio=nnratio, check_ori=bool(check_ori))


# --------------------------------------------------------------------------------------------------------------------------------
# reach: what launch_bow_seq and steps 2 / 3 of k_bow_lane decide, restated from the code
# --------------------------------------------------------------------------------------------------------------------------------
def lane_lds(cap):
    NP = 512
    while NP < cap:
        NP <<= 1
    capP = (cap + 63) & ~63
    return NP, NP * 16 + capP * (3 * 2 + 8 + 2 + 2) + NP // 32 * 12 + 64


def picks_lane_kernel(cap, nnratio):
    NP, lds = lane_lds(cap)
    return bool(cap < 65535 and NP <= 4096 and lds <= LANE_LDS_LIMIT and f32(TH) < f32(nnratio) * f32(255.0) and TH < 255)


def class_of(c2):
    return 3 if c2 > BL_MAXN2 else 0 if c2 > 64 else 1 if c2 > 16 else 2


SHAPE_OF_CLASS = {0: "J8", 1: "J4", 2: "lane", 3: "coop"}


def reach_pair(f1, f2, cap, nnratio):
    """Only what holds in every order of the atomics: whether all matrix items fit, and a lower bound of those that spill."""
    NP, lds = lane_lds(cap)
    n1, n2 = min(len(f1["desc"]), cap), min(len(f2["desc"]), cap)
    NS = 64
    while NS < max(n1, n2):
        NS <<= 1
    dcap = NP * 16 - BL_TILES * 4
    fv1, fv2 = fv_dict(f1["node"][:n1], f1["wt"][:n1]), fv_dict(f2["node"][:n2], f2["wt"][:n2])
    items = []
    for nid in sorted(set(fv1) & set(fv2)):
        r, c = len(fv1[nid]), len(fv2[nid])
        cls = class_of(c)
        tR, tC = (r + 15) >> 4, (c + 15) >> 4
        shape = SHAPE_OF_CLASS[cls] if (cls == 3 or tR <= 16) else "coop_spill"
        items.append({"node": nid, "n1": r, "n2": c, "cls": cls, "units": r * ((c + 3) >> 2), "tiles": tR * tC, "tR": tR, "shape": shape})
    mat = [it for it in items if it["cls"] != 3]

    def fit_count(key, limit):
        tot = n = 0
        for cls in (0, 1, 2):
            for x in sorted(it[key] for it in mat if it["cls"] == cls):
                tot += x
                n += tot <= limit
        return n
    units_limit = min(dcap // 4, 0xFFFE)
    best_fit = min(fit_count("units", units_limit), fit_count("tiles", BL_TILES))
    tall = sum(1 for it in mat if it["tR"] > 16)
    return {"NP": NP, "NS": NS, "dcap": dcap, "lds": lds, "kernel": "k_bow_lane" if picks_lane_kernel(cap, nnratio) else "k_bow_seq",
            "items": items, "classes": sorted(set(it["cls"] for it in items)), "shapes": sorted(set(it["shape"] for it in items)),
            "bytes": 4 * sum(it["units"] for it in mat), "tiles": sum(it["tiles"] for it in mat),
            "all_fit": best_fit == len(mat) and tall == 0, "min_spill": max(len(mat) - best_fit, tall),
            "tile_overflow": sum(it["tiles"] for it in mat) > BL_TILES, "byte_overflow": 4 * sum(it["units"] for it in mat) > dcap}


def reach(sc):
    return reach_pair(sc["f1"], sc["f2"], sc["cap"], sc["nnratio"])


# --------------------------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------------------------
def _simple_rows(nrows, n2):
    """nrows components of one row: row i has its best (20) at candidate i % n2 and nothing else below FAR"""
    return [(1, {i % n2: 20}) for i in range(nrows)]


def sc_class_edges():
    out = []
    widths = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
    for rows in (3, 1):
        p = Pair(100 + rows)
        for k, n2 in enumerate(widths):
            # the first row's best is the node's LAST candidate: the last byte / lane / trip of every width; two identical rows
            # then compete for the first and the middle candidate
            if rows == 1:
                comps = [(1, {n2 - 1: 20})]
            elif n2 == 1:
                comps = [(3, {0: 20})]
            else:
                comps = [(1, {n2 - 1: 20}), (2, {0: 25, n2 // 2: 45})]
            p.node(1000 + 10 * k, comps, n2, tag1=[("class", n2, r) for r in range(rows)])
        out.append(scene("class_edges-rows%d" % rows, "class_edges", p, 2048,
                         target={"classes": [0, 1, 2, 3], "all_fit": True, "widths": widths}))
    return out


def sc_row_edges():
    out = []
    for name, counts in (("upto256", [15, 16, 17, 255, 256]), ("257", [257])):
        for n2 in (4, 20):
            p = Pair(200 + n2 + len(counts))
            for k, nr in enumerate(counts):
                # groups of three identical rows on two candidates of their own (18, 31) while candidates last; the node's LAST row
                # is a component of its own on the last candidate, so that the first and the last row both decide something
                comps, c, left = [], 0, nr - 1
                while left > 0:
                    g = min(3, left)
                    near = {}
                    if c + 2 < n2:
                        near = {c: 18, c + 1: 31}
                        c += 2
                    comps.append((g, near))
                    left -= g
                comps.append((1, {n2 - 1: 22}))
                p.node(2000 + 7 * k, comps, n2, tag1=[("rows", nr, n2, r) for r in range(nr)])
            out.append(scene("row_edges-%s-n2_%d" % (name, n2), "row_edges", p, 1024,
                             target={"shapes": ["coop_spill"] if name == "257" else [("lane" if n2 == 4 else "J4")],
                                     "all_fit": name != "257", "min_spill": 1 if name == "257" else 0}))
    return out


def sc_tile_overflow():
    out = []
    # 40 x 40 is 3 x 3 tiles: 630 + 9 = 639 tiles just fit, 632 + 9 = 641 overflow by one
    for name, n11, big, over, spill in (("700x1", 700, False, True, 60), ("630x1+40x40", 630, True, False, 0), ("632x1+40x40", 632, True, True, 1)):
        p = Pair(300 + n11)
        for k in range(n11):
            p.node(5 + 3 * k, [(1, {0: int(k % 60)})], 1)         # distances 0 .. 59: some beyond TH
        if big:
            p.node(1, _simple_rows(40, 40), 40)
        out.append(scene("tile_overflow-" + name, "tile_overflow", p, 1024,
                         target={"tile_overflow": over, "byte_overflow": False, "all_fit": not over, "min_spill": spill}))
    return out


def _n40(p, nid, k):
    """40 x 40: 20 components of two identical rows: the first takes the 20 when 20 < 0.7 * second (second 35: yes, 27: no), and
    the second row what is left"""
    p.node(nid, [(2, {2 * i: 20, 2 * i + 1: 35 if (i + k) % 3 else 27}) for i in range(20)], 40)


def sc_matrix_overflow():
    out = []
    for cap, fit in ((512, 3), (1024, 8), (2048, 18), (4096, 39)):
        for extra in (1, 0):
            p = Pair(400 + cap + extra)
            nn = fit + extra
            for k in range(nn):
                _n40(p, 10 + 5 * k, k)
            if cap == 4096:                                        # all 4096 slots live: the rest under nodes the other side lacks
                rest = 4096 - 40 * nn
                p.node(900001, [(rest, {})], 0)
                p.node(900002, [], rest)
            out.append(scene("matrix_overflow-cap%d-%s" % (cap, "over" if extra else "fits"), "matrix_overflow", p, cap,
                             target={"byte_overflow": bool(extra), "all_fit": not extra, "min_spill": extra, "tile_overflow": False,
                                     "full": cap == 4096}))
    return out


PLACEMENT_SHAPES = {    # shape: (side-1 rows of the node, side-2 candidates, stride of the second-best reduction, positions p)
    "lane": (1, 16, 0, (0, 7, 14)),
    "J4": (1, 64, 16, (0, 7, 15)),
    "J8": (1, 128, 16, (0, 7, 15)),
    "coop": (1, 200, 64, (0, 31, 63)),
    "coop_spill": (257, 128, 64, (0, 31, 63)),
}
PLACEMENT_OFFSETS = (1, 15, 16, 32, 48, 64, 112, 128)


def sc_second_best_placement():
    """Per code shape and offset, twin nodes of one live row: best 30 at p, and in the planted twin a 40 at p + off (30 < 0.7 * 40
    fails; without the 40 the row matches).  The 257-row nodes (tR > 16: the cooperative path through spill) keep the live row last."""
    out = []
    for shape, (nrows, n2, stride, ps) in PLACEMENT_SHAPES.items():
        spill_scene, spill_nodes, spill_part = Pair(550), 0, 0
        nid = 100
        for off in PLACEMENT_OFFSETS:
            pl = [pp for pp in ps if pp + off < n2]
            if not pl:
                continue
            if nrows > 1 and spill_nodes + 2 * len(pl) > 14:         # 257 rows a node: at most 14 nodes in 4096 slots
                out.append(scene("second_best_placement-%s-part%d" % (shape, spill_part), "second_best_placement", spill_scene, 4096,
                                 target={"shapes": [shape], "all_fit": False}))
                spill_scene, spill_nodes, spill_part = Pair(551 + spill_part), 0, spill_part + 1
            p = spill_scene if nrows > 1 else Pair(500 + n2 + off)
            spill_nodes += 2 * len(pl)
            for pp in pl:
                for plant in (1, 0):
                    near = {pp: 30}
                    if plant:
                        near[pp + off] = 40
                    tag = ("place", shape, off, pp, plant)
                    if nrows == 1:
                        p.node(nid, [(1, near)], n2, tag1=[tag])
                    else:
                        p.node(nid, [(nrows - 1, {}), (1, near)], n2, tag1=[None] * (nrows - 1) + [tag])
                    nid += 3
            if nrows == 1:
                out.append(scene("second_best_placement-%s-off%d" % (shape, off), "second_best_placement", p, 2048,
                                 target={"shapes": [shape], "all_fit": True}))
        if nrows > 1:
            out.append(scene("second_best_placement-%s-part%d" % (shape, spill_part), "second_best_placement", spill_scene, 4096,
                             target={"shapes": [shape], "all_fit": False}))
    return out


def sc_greedy_order():
    """Three identical rows of a node whose best is the same candidate (distance `first`): the first claims it; the later rows have
    (a) no other candidate, (b) one other at 40, (c) two others that tie at 44.  The node's width picks the code shape.  Last, ties
    for the best at a ratio above one, the only place where the position of a tie reaches the output (a tie makes the second
    equal the best)."""
    out = []
    for first in (20, 0, 49):
        for th_mode in (0, 1):
            p = Pair(600 + first)
            nid = 50
            for n2 in (1, 2, 3, 16, 20, 64, 100, 128, 150):
                for case, others in (("a", {}), ("b", {n2 - 1: 40}), ("c", {n2 // 2: 44, n2 - 1: 44})):
                    if (n2 == 1 and others) or (n2 == 2 and case == "c"):
                        continue
                    near = dict(others)
                    near[0] = first
                    p.node(nid, [(3, near)], n2, tag1=[("greedy", case, n2, r) for r in range(3)])
                    nid += 2
            out.append(scene("greedy_order-first%d-mode%d" % (first, th_mode), "greedy_order", p, 2048, th_mode=th_mode,
                             target={"classes": [0, 1, 2, 3], "all_fit": True}))
    p = Pair(650)
    nid = 50
    for n2 in (2, 16, 20, 64, 100, 128, 150):
        for a, b in ((0, n2 - 1), (n2 // 2, n2 - 1), (0, 1)):
            if a != b:
                p.node(nid, [(2, {a: 30, b: 30})], n2, tag1=[("tie", n2, a, b)] * 2)
                nid += 2
    out.append(scene("greedy_order-ties-ratio1.25", "greedy_order", p, 2048, nnratio=1.25, target={"classes": [0, 1, 2, 3], "all_fit": True}))
    return out


def exact_ratio_pairs(nnratio):
    """(b1, b2) with b1 <= 51 where float32(nnratio) * float32(b2) is the integer b1 exactly"""
    r = f32(nnratio)
    return [(int(r * f32(b2)), b2) for b2 in range(1, 257) if float(r * f32(b2)) == int(r * f32(b2)) and 0 < int(r * f32(b2)) <= 51]


def sc_threshold_and_ratio():
    out = []
    for nnratio in (0.7, 0.75, 0.6, 0.9):
        pairs = set()
        if nnratio == 0.7:
            pairs |= {(b1, b2) for b1 in (49, 50, 51) for b2 in (70, 71, 72, 73)}
        ex = exact_ratio_pairs(nnratio)
        assert len(ex) >= 3, nnratio
        for b1, b2 in ex:
            pairs |= {(b1, b2), (b1 - 1, b2), (b1 + 1, b2)} if b1 + 1 < b2 else {(b1, b2)}
        pairs = sorted(x for x in pairs if 0 <= x[0] < x[1])
        for th_mode in (0, 1):
            p = Pair(700 + int(nnratio * 100))
            nid = 10
            for b1, b2 in pairs:
                for n2 in (2, 20):                                  # a lane item and a row item
                    p.node(nid, [(1, {n2 - 1: b1, 0: b2})], n2, tag1=[("ratio", b1, b2, n2)])
                    nid += 1
            out.append(scene("threshold_and_ratio-%g-mode%d" % (nnratio, th_mode), "threshold_and_ratio", p, 4096, th_mode=th_mode,
                             nnratio=nnratio, target={"exact": ex, "all_fit": True}))
    return out


def clamp_bound_ratios():
    """the smallest float32 r with 50 < r * 255 in float32, and its predecessor"""
    r = f32(50.0) / f32(255.0)
    while not (f32(TH) < r * f32(255.0)):
        r = np.nextafter(r, f32(1))
    while f32(TH) < np.nextafter(r, f32(0)) * f32(255.0):
        r = np.nextafter(r, f32(0))
    return float(r), float(np.nextafter(r, f32(0)))


def sc_clamp_bound():
    """Rows with best 49 / 50 whose second best is 253 .. 256 away (every other candidate of the node at that distance), a lone
    candidate, or nothing but claimed candidates: the byte matrix reads 255 where the reference reads 256 or skips."""
    out = []
    for which, r in zip(("at", "below"), clamp_bound_ratios()):
        for th_mode in (0, 1):
            p = Pair(800)
            nid = 10
            for b1 in (49, 50):
                for w in (2, 17, 70, 130):
                    for second in (253, 254, 255, 256):
                        near = {c: second for c in range(w)}
                        near[w // 2] = b1
                        p.node(nid, [(1, near)], w, tag1=[("clamp", b1, second, w)])
                        nid += 1
                p.node(nid, [(1, {0: b1})], 1, tag1=[("clamp", b1, "lone", 1)])
                nid += 1
                for K in (1, 3, 16, 20):                            # K rows claim K candidates (distance 0); the last row's own is left
                    comps = [(1, {c: 0}) for c in range(K)] + [(1, {K: b1})]
                    p.node(nid, comps, K + 1, tag1=[("clamp", 0, "claims", K + 1)] * K + [("clamp", b1, "claimed", K + 1)])
                    nid += 1
            out.append(scene("clamp_bound-%s-mode%d" % (which, th_mode), "clamp_bound", p, 2048, th_mode=th_mode, nnratio=r,
                             target={"kernel": "k_bow_lane" if which == "at" else "k_bow_seq"}))
    return out


def _valid_patterns(n):
    return {"first": [0] + [1] * (n - 1), "last": [1] * (n - 1) + [0], "alternate": [i & 1 for i in range(n)], "all": [0] * n}


def sc_validity():
    out = []
    """The 258-row nodes (tR > 16) set s_over and take their bytes in the matrix prefix whether they fit or not, so they stay in a
    scene of their own: in the other scene every item fits and each matrix shape runs its own invalid rows."""
    shapes = (("lane", 6, 8), ("J4", 6, 40), ("J8", 6, 100), ("coop", 6, 140), ("coop_spill", 258, 30))
    for th_mode, group in ((m, g) for m in (0, 1) for g in (shapes[:4], shapes[4:])):
        p = Pair(900 + len(group))
        nid = 10
        for shape, nr, n2 in group:
            for pat in ("first", "last", "alternate", "all"):
                # pairs of identical rows compete for (18, 31): an invalid first row hands its candidate to the second
                comps = [(2, {2 * i: 18, 2 * i + 1: 31}) for i in range(min(nr // 2, n2 // 2))]
                live = sum(g for g, _ in comps)
                if live < nr:
                    comps.append((nr - live, {}))
                v1 = _valid_patterns(nr)[pat]
                # valid2: the candidate that would win the first pair of rows is invalid
                v2 = [1] * n2
                v2[0] = 0
                p.node(nid, comps, n2, v1=v1, v2=v2, tag1=[("valid", shape, pat, r) for r in range(nr)])
                nid += 1
        spill = group[0][0] == "coop_spill"
        out.append(scene("validity-%smode%d" % ("257rows-" if spill else "", th_mode), "validity", p, 2048, th_mode=th_mode,
                         use_valid=True, target={"shapes": sorted(g[0] for g in group), "all_fit": not spill, "min_spill": 4 if spill else 0}))
    # the same descriptors with no valid pointer at all
    p = Pair(900)
    nid = 10
    for shape, nr, n2 in shapes[:4]:
        comps = [(2, {2 * i: 18, 2 * i + 1: 31}) for i in range(min(nr // 2, n2 // 2))]
        p.node(nid, comps, n2, v1=[0] * nr, v2=[0] * n2, tag1=[("valid", shape, "null", r) for r in range(nr)])
        nid += 1
    for th_mode in (0, 1):
        out.append(scene("validity-null-mode%d" % th_mode, "validity", p, 1024, th_mode=th_mode, use_valid=False,
                         target={"shapes": ["J4", "J8", "coop", "lane"], "all_fit": True}))
    return out


STOP_WEIGHTS = (0.0, -0.0, -1.0, float("nan"), 1e-45, 1e-38)


def sc_stopped_features():
    p = Pair(1000)
    nid = 10
    for wi, w in enumerate(STOP_WEIGHTS):
        for n2 in (3, 20, 70, 130):
            # on the feature that would win (side 2), with a runner-up the row takes instead
            w2 = [1.0] * n2
            w2[0] = w
            p.node(nid, [(1, {0: 10, n2 - 1: 30})], n2, w2=w2, tag1=[("stop", wi, "winner", n2)])
            nid += 1
            # on the row itself
            if n2 <= 20:
                p.node(nid, [(1, {0: 10})], n2, w1=[w], tag1=[("stop", wi, "row", n2)])
                nid += 1
        # all features of a node on one side
        p.node(nid, [(2, {0: 10, 1: 12})], 4, w1=[w, w], tag1=[("stop", wi, "side1", 4)] * 2)
        nid += 1
        p.node(nid, [(2, {0: 10, 1: 40})], 4, w2=[w] * 4, tag1=[("stop", wi, "side2", 4)] * 2)
        nid += 1
    return [scene("stopped_features", "stopped_features", p, 2048, target={"classes": [0, 1, 2, 3]})]


def sc_node_ids():
    """Ids 0, 1, 2^31 - 2, 2^31 - 1 and runs of adjacent ids.  All nodes but two carry the same content, so that two nodes a defect
    merges show duplicates (a tie for the best: the ratio test fails where it passed)."""
    p = Pair(1100)
    T = (1 << 31) - 1
    shared = [0, 1, 2, 3, 4, 10, 11, 12, 0x3FFFFFFE, 0x3FFFFFFF, 0x40000000, T - 3, T - 2, T - 1, T]
    for k, nid in enumerate(shared):
        p.node(nid, [(2, {k % 3: 15, 3: 45})], 4, tag1=[("ids", nid, r) for r in range(2)], content=k % 3 if nid in (4, 12) else 0)
    # ids on one side only, between shared ones
    for nid in (5, 7, 9, 0x3FFFFFFD, T - 5):
        p.node(nid, [(2, {})], 0)
    for nid in (6, 8, 13, 0x40000001, T - 4):
        p.node(nid, [], 3)
    return [scene("node_ids", "node_ids", p, 512, target={"all_fit": True})]


def half_rotations():
    """float32 rotations whose bin value rot * (1 / 30.f) is exactly m + 0.5 with m even: roundf goes up, half-to-even goes down"""
    out = []
    c = f32(1.0) / f32(30)
    for m in (0, 2, 4, 6, 8, 10):
        r0 = f32(30 * (m + 0.5))
        for step in sorted(range(-8, 9), key=abs):
            r = r0
            for _ in range(abs(step)):
                r = np.nextafter(r, f32(1000 if step > 0 else -1000))
            if float(f32(r * c)) == m + 0.5:
                out.append((m, float(r)))
                break
    return out


def _rot_scene(name, bins, extra=(), check_ori=1):
    """bins: {bin: count} of certain matches (1 x 1 nodes, distance 0) whose rotation is 30 * bin; extra: (angle1, angle2, tag)"""
    p = Pair(1200)
    nid = 10
    for b, cnt in sorted(bins.items()):
        for k in range(cnt):
            a2 = float(k % 7) * 30.0
            a1 = a2 + (30.0 * b if b < 12 else 350.0)               # (bin 12 is 345 .. 360)
            if a1 >= 360.0:                                         # a negative difference: + 360 lands in the same bin
                a1, a2 = a1 - 360.0, a2
            p.node(nid, [(1, {0: 0})], 1, a1=[a1], a2=[a2], tag1=[("rot", b, k)])
            nid += 1
    for a1, a2, tag in extra:
        p.node(nid, [(1, {0: 0})], 1, a1=[a1], a2=[a2], tag1=[tag])
        nid += 1
    return scene(name, "rotation", p, 512, check_ori=check_ori, target={"bins": bins})


def sc_rotation():
    out = []
    for co in (1, 0):
        sfx = "" if co else "-noori"
        out.append(_rot_scene("rotation-tie3" + sfx, {2: 5, 5: 5, 9: 5, 11: 3}, check_ori=co))
        out.append(_rot_scene("rotation-tie4" + sfx, {1: 4, 3: 4, 6: 4, 8: 4, 10: 1}, check_ori=co))
        for max1 in (10, 20, 30):
            at = max1 // 10
            for m2, m3 in ((at, at), (at + 1, at), (at + 1, at - 1), (at, at - 1), (at - 1, at - 1), (at + 1, at + 1)):
                bins = {4: max1, 7: m2, 1: m3, 12: 1}
                out.append(_rot_scene("rotation-cut%d-%d-%d%s" % (max1, m2, m3, sfx), {b: c for b, c in bins.items() if c > 0}, check_ori=co))
        extra = [(15.0, 0.0, ("rotx", 15)), (45.0, 0.0, ("rotx", 45)), (345.0, 0.0, ("rotx", 345)), (-0.0, 0.0, ("rotx", -0.0)),
                 (0.0, 1e-6, ("rotx", "neg360")), (10.0, 355.0, ("rotx", "neg15"))]
        out.append(_rot_scene("rotation-exact" + sfx, {1: 3, 2: 3, 12: 3, 0: 3}, extra, check_ori=co))
        for m, r in half_rotations():
            # the half match belongs to bin m + 1 (kept: 5 + 1 there); rounded to even it lands in bin m (1 match: cut)
            others = [b for b in (3, 7, 11, 9) if b not in (m, m + 1)][:2]
            bins = {m + 1: 5, others[0]: 8, others[1]: 8}
            out.append(_rot_scene("rotation-half%d%s" % (m, sfx), bins, [(r, 0.0, ("half", m))], check_ori=co))
    return out


def sc_shapes():
    """(n1, n2) at the ends of cap; every feature under one of a few shared nodes so that the counts decide the work"""
    out = []
    for cap in (64, 65, 512, 513, 4096):
        combos = [(cap, cap), (cap, 1), (1, cap), (0, cap), (cap, 0)]
        if cap == 513:
            combos += [(512, 513), (513, 512)]
        for n1, n2 in combos:
            p = Pair(1300 + cap)
            nn = max(1, min(n1, n2, cap // 8))                      # shared nodes
            for k in range(nn):
                r = n1 // nn + (1 if k < n1 % nn else 0)
                c = n2 // nn + (1 if k < n2 % nn else 0)
                live = min(r, c // 2, 3)
                comps = [(1, {2 * i: 18, 2 * i + 1: 31 + i}) for i in range(live)]
                if r and c == 1:
                    live, comps = 1, [(1, {0: 18})]
                if r > live:
                    comps.append((r - live, {}))
                # (the one-sided frame's node has an id of its own: the cross pair with the one-sided frame before it would be one
                # node of cap x cap, 16 M distances in the Python model for nothing this family is about)
                if r or c:
                    p.node((10 if n2 else 5000) + k, comps, c)
            tall = nn == 1 and n1 > 256 and n2 > 0                  # one node of cap rows: tR > 16, the cooperative path through spill
            out.append(scene("shapes-cap%d-%dx%d" % (cap, n1, n2), "shapes", p, cap,
                             target={"n": (n1, n2), "all_fit": not tall, "shapes": ["coop_spill"]} if tall else {"n": (n1, n2), "all_fit": True}))
    return out


FAMILIES = {"class_edges": sc_class_edges, "row_edges": sc_row_edges, "tile_overflow": sc_tile_overflow,
            "matrix_overflow": sc_matrix_overflow, "second_best_placement": sc_second_best_placement, "greedy_order": sc_greedy_order,
            "threshold_and_ratio": sc_threshold_and_ratio, "clamp_bound": sc_clamp_bound, "validity": sc_validity,
            "stopped_features": sc_stopped_features, "node_ids": sc_node_ids, "rotation": sc_rotation, "shapes": sc_shapes}
_cache = {}


def scenes(family):
    if family not in _cache:
        _cache[family] = FAMILIES[family]()
    return _cache[family]


# the scenes each variant must be told apart on, and the floor (rows of side 1 whose match differs)
VARIANT_FAMILIES = {"second_skips_own_lane": ("second_best_placement",), "second_skips_own_lane64": ("second_best_placement",),
                    "claimed_is_candidate": ("greedy_order",), "claimed_reads_255": ("clamp_bound",), "dist_clamped_255": ("clamp_bound",),
                    "le_for_lt": ("threshold_and_ratio",), "lt_for_le": ("threshold_and_ratio",), "ratio_in_double": ("threshold_and_ratio",),
                    "tie_takes_highest": ("greedy_order",), "valid2_in_mode0": ("validity",), "stopped_kept": ("stopped_features",),
                    "nan_weight_kept": ("stopped_features",), "node_ids_truncated": ("node_ids",), "adjacent_ids_merged": ("node_ids",),
                    "maxima_ge": ("rotation",), "cut_in_double": ("rotation",), "round_half_even": ("rotation",)}
FLOOR = 3


# --------------------------------------------------------------------------------------------------------------------------------
# batches
# --------------------------------------------------------------------------------------------------------------------------------
def _frame_arrays(frames, cap):
    B = len(frames)
    desc = np.zeros((B, cap, 32), np.uint8)
    node = np.zeros((B, cap), np.int32)
    wt = np.zeros((B, cap), f32)
    valid = np.zeros((B, cap), np.uint8)
    angle = np.zeros((B, cap), f32)
    counts = np.zeros(B, np.int32)
    for b, f in enumerate(frames):
        n = len(f["desc"])
        assert n <= cap
        counts[b] = n
        desc[b, :n], node[b, :n], wt[b, :n], valid[b, :n], angle[b, :n] = f["desc"], f["node"], f["wt"], f["valid"], f["angle"]
    return {"desc": desc, "node": node, "wt": wt, "valid": valid, "angle": angle, "counts": counts}


def batches(family):
    """Scenes that share (cap, th_mode, nnratio, check_ori, valid pointer) as frames 2k, 2k + 1 of one batch with lag 1; the cross
    pairs (2k + 1, 2k + 2) are checked against the oracle too."""
    groups = {}
    for sc in scenes(family):
        key = (sc["cap"], sc["th_mode"], sc["nnratio"], sc["check_ori"], sc["use_valid"])
        groups.setdefault(key, []).append(sc)
    out = []
    for (cap, th_mode, nnratio, check_ori, use_valid), scs in sorted(groups.items(), key=lambda kv: kv[0]):
        frames = []
        for sc in scs:
            frames += [sc["f1"], sc["f2"]]
        b = _frame_arrays(frames, cap)
        b.update({"name": "%s-cap%d-mode%d-r%.9g-ori%d-valid%d" % (family, cap, th_mode, nnratio, check_ori, use_valid), "frames": frames,
                  "cap": cap, "lag": 1, "th_mode": th_mode, "nnratio": nnratio, "check_ori": check_ori, "use_valid": use_valid,
                  "scenes": [s["name"] for s in scs]})
        out.append(b)
    return out


def lag_batches():
    """B = 3 frames at lag 0 .. 3 (lag 0: a frame against itself; lag 3: no frame has a predecessor), and counts beyond cap."""
    out = []
    scs = scenes("class_edges") + scenes("greedy_order")[:1]
    frames = [scs[0]["f1"], scs[0]["f2"], scs[2]["f2"]]
    for lag in (0, 1, 2, 3):
        b = _frame_arrays(frames, 2048)
        b.update({"name": "shapes-lag%d" % lag, "frames": frames, "cap": 2048, "lag": lag, "th_mode": 0, "nnratio": float(f32(0.7)),
                  "check_ori": 1, "use_valid": False, "scenes": []})
        out.append(b)
    for cap in (64, 513):
        full = [s for s in scenes("shapes") if s["name"] == "shapes-cap%d-%dx%d" % (cap, cap, cap)][0]
        frames = [full["f1"], full["f2"], full["f1"]]
        b = _frame_arrays(frames, cap)
        b["counts"][:] = cap + 7                                    # more features than slots: the pair at cap features
        b.update({"name": "shapes-counts-beyond-cap%d" % cap, "frames": frames, "cap": cap, "lag": 1, "th_mode": 0,
                  "nnratio": float(f32(0.7)), "check_ori": 1, "use_valid": False, "scenes": []})
        out.append(b)
    return out


def all_batches(family):
    return batches(family) + (lag_batches() if family == "shapes" else [])


def expected(oracle, batch):
    """The oracle's (nmatches, match12, match21) per frame of the batch; None for frames with no predecessor.  Cached on the batch."""
    if "want" not in batch:
        fr, lag = batch["frames"], batch["lag"]
        batch["want"] = [None if b < lag else oracle_pair(oracle, fr[b - lag], fr[b], batch["th_mode"], batch["nnratio"],
                                                          batch["check_ori"], batch["use_valid"]) for b in range(len(fr))]
    return batch["want"]
