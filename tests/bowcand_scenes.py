"""Scenes for SearchByBoW against candidate key frames: sides in the form tests/bowcand_model.py takes, with low-entropy descriptors
(16 random bits, or "the first k bits set") so that equal distances, the ratio test and the order of the lists decide.  A scene is
(fixed, [candidate, ...], params): params holds th / nnratio / check_ori where a scene needs other values than the reference's.
A side that appears twice in the list is the same candidate twice.  tests/test_bowcand_model.py checks that every named scene
yields what its name says."""
import numpy as np

import bowcand_model as M

f32 = np.float32
ANGLES = np.asarray([0.0, 12.0, 31.0, 95.5, 180.5, 270.0, 359.0], f32)
NLEVELS = 8
SIGMA2 = np.asarray([f32(1.2) ** (2 * l) for l in range(NLEVELS)], f32)


def bits(k, extra=()):
    """A descriptor with the first k bits set (and the bits of `extra`): distance(bits(a), bits(b)) == |a - b|."""
    b = np.zeros(256, np.uint8)
    b[:k] = 1
    for e in extra:
        b[e] ^= 1
    return np.packbits(b)


def random_side(rng, nodes, p_none=0.15, p_bad=0.1, spare=0):
    """nodes: {node id: number of features}; `spare` features belong to no node.  Features go to nodes in a random order, so a
    node's list is neither ascending nor contiguous."""
    n = sum(nodes.values()) + spare
    perm = [int(i) for i in rng.permutation(n)]
    fv, at = {}, 0
    for g, cnt in nodes.items():
        fv[g] = perm[at:at + cnt]
        at += cnt
    desc = np.zeros((n, 32), np.uint8)
    desc[:, :2] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    pts = []
    for i in range(n):
        r = rng.random()
        pts.append(None if r < p_none else M.Point(r < p_none + p_bad, tuple(rng.standard_normal(3).astype(f32))))
    return {"desc": desc, "angle": rng.choice(ANGLES, n).astype(f32), "x": (rng.random(n) * 640).astype(f32),
            "y": (rng.random(n) * 480).astype(f32), "octave": rng.integers(0, NLEVELS, n).astype(np.int32), "fv": fv, "points": pts}


def craft_side(nodes, angles=None, good=None, octaves=None):
    """nodes: {node id: [descriptor, ...]} in list order.  Feature indices run AGAINST the list order (the first list entry of the
    first node has the highest index), so a lower list position never coincides with a lower feature index.  angles / good /
    octaves: {node id: [...]} beside nodes (default 0.0 / a good point / octave 0); good False = no point, "bad" = a bad one."""
    n = sum(len(v) for v in nodes.values())
    desc, angle, octave, pts, fv = np.zeros((n, 32), np.uint8), np.zeros(n, f32), np.zeros(n, np.int32), [None] * n, {}
    i = n
    for g in sorted(nodes):
        fv[g] = []
        for p, d in enumerate(nodes[g]):
            i -= 1
            desc[i] = d
            angle[i] = (angles or {}).get(g, [0.0] * len(nodes[g]))[p]
            octave[i] = (octaves or {}).get(g, [0] * len(nodes[g]))[p]
            ok = (good or {}).get(g, [True] * len(nodes[g]))[p]
            pts[i] = None if ok is False else M.Point(ok == "bad", (f32(i), f32(g), f32(p + 0.5)))
            fv[g].append(i)
    return {"desc": desc, "angle": angle, "x": (np.arange(n) * 3 + 1).astype(f32), "y": (np.arange(n) * 2 + 0.5).astype(f32),
            "octave": octave, "fv": fv, "points": pts}


def as_scene(mode, side1, sides2, **params):
    """A pair (side 1, side 2) as a call: mode 0 has the candidate on side 1 and the frame on side 2, mode 1 the reverse, so a
    scene with several sides 2 is a mode-1 scene and one with several sides 1 a mode-0 scene."""
    if mode == 0:
        assert len(sides2) == 1
        return sides2[0], [side1], params
    return side1, list(sides2), params


# ---- node sizes: the three paths of the node body and their edges; the 64-feature chunk of side 1 ----
def node_sizes(mode, n2, n1=3, seed=0):
    """One shared node with n2 features on side 2 and n1 on side 1, a second ordinary node beside it, and a node only one side has."""
    rng = np.random.default_rng(1000 * n2 + n1 + seed)
    s1 = random_side(rng, {4: n1, 9: 5, 11: 2}, spare=2)
    s2 = random_side(rng, {4: n2, 9: 6, 30: 3}, spare=1)
    if n2:
        # so that the node under test matches whatever its size: the first two side-1 features of its list are near twins of ONE
        # side-2 feature from the middle of its list (the second has to do with what the first left), the last side-1 feature
        # is the near twin of the LAST side-2 feature of the list
        l1, l2 = s1["fv"][4], s2["fv"][4]
        good = M.Point(False, (f32(1), f32(2), f32(3)))
        for a, b, byte in ((l1[0], l2[n2 // 2], 31), (l1[1], l2[n2 // 2], 30), (l1[-1], l2[-1], 31)):
            s1["desc"][a] = s2["desc"][b]
            s1["desc"][a][byte] = 1
            s1["points"][a] = s2["points"][b] = good
    return as_scene(mode, s1, [s2])


def node4_matches(mode, scene):
    """How many matches the node under test (4) of a node_sizes scene gives without the rotation check."""
    fixed, cands, _ = scene
    row = M.candidates(mode, fixed, cands, check_ori=False)["matches"][0]
    side_of_row, other = fixed, cands[0]
    return sum(1 for i in side_of_row["fv"][4] if row[i] >= 0 and row[i] in other["fv"][4])


def batch(mode, K, seed=0, nodes_per_cand=(3, 5, 2, 7, 1, 6, 3, 5, 9)):
    """K candidates whose shared-node counts are no multiple of four, so the pairs of one candidate straddle a block of four waves;
    candidate k shares nodes_per_cand[k] nodes with the fixed side."""
    rng = np.random.default_rng(77 + K + seed)
    fixed = random_side(rng, {g: int(rng.integers(1, 9)) for g in range(2, 40, 3)}, spare=3)
    cands = []
    for k in range(K):
        shared = [int(g) for g in rng.choice(sorted(fixed["fv"]), nodes_per_cand[k % len(nodes_per_cand)], replace=False)]
        nodes = {g: int(rng.integers(1, 9)) for g in shared}
        nodes.update({g: 2 for g in (1, 41 + k)})     # nodes the fixed side does not have
        cands.append(random_side(rng, nodes, spare=1))
    return fixed, cands, {}


def twice(mode):
    fixed, cands, p = batch(mode, 3, seed=5)
    return fixed, [cands[0], cands[1], cands[0], cands[2]], p


def disjoint(mode):
    """The middle candidate shares no node with the fixed side."""
    fixed, cands, p = batch(mode, 3, seed=9)
    rng = np.random.default_rng(3)
    cands[1] = random_side(rng, {1: 4, 100: 5})
    return fixed, cands, p


# ---- thresholds and ties (one node, hand-made distances) ----
def threshold(mode, th=8):
    """Best distance exactly th, the second best far enough for the ratio: a match in mode 0 (<=), none in mode 1 (<)."""
    return as_scene(mode, craft_side({7: [bits(0)]}), [craft_side({7: [bits(20), bits(th)]})], th=th)


def ratio_equal(mode, second=4):
    """(float)3 < 0.75f * (float)4 is false: no match at equality.  second=5: the neighbouring case that matches."""
    return as_scene(mode, craft_side({7: [bits(0)]}), [craft_side({7: [bits(3), bits(second)]})], nnratio=0.75)


def tie(mode):
    """Two side-2 features at the same best distance; with nnratio 1.5 the ratio passes and the lower list position wins."""
    return as_scene(mode, craft_side({7: [bits(0)]}), [craft_side({7: [bits(9), bits(2), bits(1, extra=(5,)), bits(6)]})], nnratio=1.5)


def claimed(mode):
    """Side-1 features A then B of one node both prefer X; A claims it, B has to take Y."""
    return as_scene(mode, craft_side({7: [bits(0), bits(1)]}), [craft_side({7: [bits(10), bits(2)]})])


# ---- rotation: every node one feature a side at distance 1, the angles make the histogram ----
def rotation(mode, rots):
    """One match per entry of rots with angle1 - angle2 = that value (angle2 = 0)."""
    n = len(rots)
    s1 = craft_side({g: [bits(0)] for g in range(n)}, angles={g: [f32(r)] for g, r in enumerate(rots)})
    s2 = craft_side({g: [bits(1)] for g in range(n)})
    return as_scene(mode, s1, [s2])


def rot_two_bins(mode):
    return rotation(mode, [0, 0, 0, 95, 95])


def rot_second_below_tenth(mode):
    """Eleven matches in bin 0 and one in bin 3: 1 < 0.1f * 11, the single one goes."""
    return rotation(mode, [0] * 11 + [95])


def rot_bin_30(mode):
    """rot = 900: round(900 / 30) = 30 -> bin 0, beside five matches of bin 6, four of bin 9 and one of bin 3 (the loser)."""
    return rotation(mode, [900, 180, 180, 180, 180, 180, 270, 270, 270, 270, 95])


# ---- validity ----
def all_invalid(mode):
    """Every feature of the candidate without a point, or with a bad one."""
    fixed, cands, p = node_sizes(mode, 6, 5)
    cands[0]["points"] = [None if i % 2 else M.Point(True, (f32(0), f32(0), f32(0))) for i in range(len(cands[0]["points"]))]
    return fixed, cands, p


# ---- gather (mode 0): octaves 0 and NLEVELS - 1 among the matched frame features ----
def gather_scene(n=6):
    s1 = craft_side({g: [bits(0)] for g in range(n)})
    s2 = craft_side({g: [bits(1)] for g in range(n)}, octaves={g: [0 if g % 2 else NLEVELS - 1] for g in range(n)})
    few = craft_side({g: [bits(0)] for g in range(n - 1)})
    return s2, [s1, few, s1], {}
