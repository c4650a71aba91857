"""Seeded vocabulary trees of the kind DBoW2 builds, and a model of the transform over them.

orbhip.distributed.make_synthetic_vocabulary makes complete k-ary trees numbered level by level with weights in (0, 1).  A tree
that TemplatedVocabulary::create builds (ref: Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) differs in every one of these:
  * HKmeansStep gives a node fewer than k children when few descriptors reach it (:696), and k may be as large as 20 (:1585);
  * it stops above level L where a cluster holds one descriptor (:849), so leaves lie at every depth;
  * it numbers a node's children consecutively and only then descends into each of them (:825, :851), so ids are in creation
    order, not level order, and the children of a node are not the ids that follow it;
  * sibling clusters can be equal or one bit apart (the first child wins a tie, :1470);
  * IDF weighting gives words of weight 0, which transform drops (:1334).
make_tree builds such a tree out of explicit node objects and packs them with distributed.pack_vocabulary; model_transform is the
descent of :1443-1485 over those objects with Python integers -- it never reads the blob, so a misreading of the file format that
the oracle's loader and the library's share shows as a difference.  Pure Python and numpy, no device."""
import numpy as np

FANOUTS = (1, 2, 3, 9, 10, 11, 13, 19, 20)     # of inner nodes below the root; the root has kmax children
ROOT_LEAVES = 3                                # children of the root that stay leaves (depth 1)
STOP_ZERO, STOP_NEG = 0.10, 0.04               # share of the leaves with weight 0.0 / a negative weight
TARGET_NODES = 8000


class Node:
    __slots__ = ("id", "parent", "depth", "desc", "weight", "children", "word")

    def __init__(self, nid, parent, depth, desc):
        self.id, self.parent, self.depth, self.desc = nid, parent, depth, desc
        self.weight = np.float32(0)
        self.children = []
        self.word = -1


def _to_int(d):
    return int.from_bytes(np.asarray(d, np.uint8).tobytes(), "little")


def _to_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def _flip(rng, v, nbits):
    for b in rng.choice(256, int(nbits), replace=False):
        v ^= 1 << int(b)
    return v


def _grow_probability(L, kmax):
    """The share of the nodes at depths 2 .. L-1 that get children, such that the tree has about TARGET_NODES nodes."""
    if L <= 2:
        return 0.0
    m = sum(FANOUTS) / len(FANOUTS)
    base = kmax + (kmax - ROOT_LEAVES) * m      # depths 1 and 2

    def total(g):
        return kmax + (kmax - ROOT_LEAVES) * m * sum((g * m) ** i for i in range(L - 1))
    lo, hi = 0.0, 1.0
    if total(1.0) <= TARGET_NODES or base >= TARGET_NODES:
        return 1.0 if base < TARGET_NODES else 0.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if total(mid) < TARGET_NODES else (lo, mid)
    return lo


def make_tree(seed, L, kmax=20, pool=None):
    """-> (nodes, blob): nodes[id] for id 0 (the root) .. n, and the binary vocabulary (k = kmax, scoring L1, weighting TF_IDF).

    Without a pool a child's descriptor is its parent's with a few dozen bits flipped (fewer further down), so that a probe made
    from a node's descriptor finds its way to that node; with a pool [m][32] every node's descriptor is a pool entry with up to
    three bits flipped.  Either way a quarter of the siblings then copy an earlier sibling and a sixth differ from one by a single
    bit, and fixed pairs are made equal: positions 9 and 10 (the two trips of the kernels' child loop), 0 and 10 (the same slot of
    both trips), 0 and 1 (the two child columns of a quad), 0 and 2 (one column, successive loads)."""
    rng = np.random.default_rng(seed)
    pool_int = None if pool is None else [_to_int(d) for d in np.asarray(pool, np.uint8).reshape(-1, 32)]
    grow = _grow_probability(L, kmax)
    nodes = [Node(0, 0, 0, 0)]
    counter = {"inner": 0, "wide": 0}

    def fresh(parent_desc, depth):
        if pool_int is not None:
            return _flip(rng, pool_int[int(rng.integers(len(pool_int)))], rng.integers(0, 4))
        if depth == 1:
            return _to_int(rng.integers(0, 256, 32, dtype=np.uint8))
        return _flip(rng, parent_desc, max(36 - 8 * depth, 6) + int(rng.integers(0, 5)))

    def step(parent, depth):                                 # HKmeansStep(parent_id, ..., current_level = depth)
        if parent.id == 0:
            f = kmax
        else:
            f = FANOUTS[(counter["inner"] + int(rng.integers(0, 2))) % len(FANOUTS)]
            counter["inner"] += 1
        descs = [fresh(parent.desc, depth) for _ in range(f)]
        for j in range(1, f):
            r = rng.random()
            if r < 0.25:
                descs[j] = descs[int(rng.integers(0, j))]
            elif r < 0.40:
                descs[j] = descs[int(rng.integers(0, j))] ^ (1 << int(rng.integers(0, 256)))
        if f >= 11:
            if counter["wide"] % 2 == 0:
                descs[10] = descs[9]
            else:
                descs[10] = descs[0]
            counter["wide"] += 1
        if f >= 3 and counter["inner"] % 3 == 1:
            descs[2] = descs[0]
            if descs[1] == descs[0]:
                descs[1] = descs[0] ^ 1
        elif f >= 2 and counter["inner"] % 3 == 2:
            descs[1] = descs[0]
        first = len(nodes)
        for j in range(f):                                   # the children get consecutive ids (:822-829) ...
            nodes.append(Node(first + j, parent.id, depth, descs[j]))
            parent.children.append(first + j)
        if depth < L:                                        # ... and only then each child's subtree (:832-853)
            stay = set(int(v) for v in rng.choice(f, ROOT_LEAVES, replace=False)) if parent.id == 0 else None
            for j in range(f):
                go = (j not in stay) if stay is not None else (rng.random() < grow)
                if go:
                    step(nodes[first + j], depth + 1)

    step(nodes[0], 1)
    words = 0
    for nd in nodes[1:]:
        nd.weight = np.float32(rng.random() * 0.98 + 0.01)
        if not nd.children:                                  # words are numbered in id order among the leaves
            nd.word = words
            words += 1
            r = rng.random()
            if r < STOP_ZERO:
                nd.weight = np.float32(0.0)
            elif r < STOP_ZERO + STOP_NEG:
                nd.weight = np.float32(-0.25)
    from orbhip import distributed as D
    body = nodes[1:]
    blob = D.pack_vocabulary(kmax, L, 0, 0, np.array([nd.parent for nd in body], np.int32),
                             np.stack([_to_bytes(nd.desc) for nd in body]), np.array([nd.weight for nd in body], np.float32),
                             np.array([0 if nd.children else 1 for nd in body], np.uint8))
    return nodes, blob


def _descend(nodes, feat):
    """TemplatedVocabulary.h:1455-1480: -> (ids of the nodes chosen at levels 1, 2, ..., whether a level's smallest distance was
    shared by two children)."""
    path, tie, cur = [], False, nodes[0]
    while True:
        best_d, best = None, None
        for cid in cur.children:                             # strict '<' in child order: the first child wins a tie
            d = bin(feat ^ nodes[cid].desc).count("1")
            if best_d is None or d < best_d:
                best_d, best, shared = d, cid, False
            elif d == best_d:
                shared = True
        tie = tie or shared
        cur = nodes[best]
        path.append(best)
        if not cur.children:
            return path, tie


def model_transform(nodes, L, desc, levelsup):
    """TemplatedVocabulary::transform (:1443-1485) of every row of desc [n][32] over the node objects -> dict of arrays: word,
    weight (float32), node (the node id at level L - levelsup; 0 when that level is <= 0 and -- the oracle's canonical choice
    for the value the reference leaves unset -- when the leaf lies above it), depth (of the leaf), tie."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    out = dict(word=np.empty(n, np.int32), weight=np.empty(n, np.float32), node=np.empty(n, np.int32),
               depth=np.empty(n, np.int32), tie=np.empty(n, bool))
    nid_level = L - levelsup
    for i in range(n):
        path, tie = _descend(nodes, _to_int(desc[i]))
        leaf = nodes[path[-1]]
        out["word"][i], out["weight"][i] = leaf.word, leaf.weight
        out["node"][i] = path[nid_level - 1] if 0 < nid_level <= len(path) else 0
        out["depth"][i], out["tie"][i] = len(path), tie
    return out


def probe_descriptors(nodes, n, seed):
    """[n][32]: half random, half a random node's descriptor with 0 .. 19 bits flipped, ordered so that neighbours in index end
    at leaves of different depths (the lanes of a wave leave the descent at different levels)."""
    rng = np.random.default_rng(seed)
    ints = []
    for i in range(n):
        if i % 2:
            ints.append(_to_int(rng.integers(0, 256, 32, dtype=np.uint8)))
        else:
            ints.append(_flip(rng, nodes[int(rng.integers(1, len(nodes)))].desc, rng.integers(0, 20)))
    depth = np.array([len(_descend(nodes, v)[0]) for v in ints])
    key = np.empty(n)
    for d in np.unique(depth):
        idx = np.nonzero(depth == d)[0]
        key[idx] = (np.arange(len(idx)) + 0.5) / len(idx)
    order = np.argsort(key, kind="stable")
    return np.stack([_to_bytes(ints[i]) for i in order])


_CASES = {}


def tree_case(seed, L=4, nprobe=1200):
    """The tree of a seed with its probe set, made once per process and shared (read-only) by the tests that use it."""
    key = (seed, L, nprobe)
    if key not in _CASES:
        nodes, blob = make_tree(seed, L)
        probes = probe_descriptors(nodes, nprobe, seed + 1000)
        probes.setflags(write=False)
        _CASES[key] = dict(nodes=nodes, blob=blob, L=L, probes=probes, model={})
    return _CASES[key]


def case_model(case, levelsup):
    """model_transform of the case's probes, computed once per levelsup."""
    if levelsup not in case["model"]:
        m = model_transform(case["nodes"], case["L"], case["probes"], levelsup)
        for a in m.values():
            a.setflags(write=False)
        case["model"][levelsup] = m
    return case["model"][levelsup]
