"""Independent model of the covisibility graph (ref: src/KeyFrame.cc:528-562 AddConnection / UpdateBestCovisibles, :731-843
UpdateConnections), written on the observation maps of tests/localmap_collect_model.py's World: for every point of the key frame
the walk goes over the point's own key frame -> index map, as the reference's does.  It does not intersect key-frame rows: that is
the formulation of the kernels under test.  Keys stand for pointers and for mnId + 1; orders that the reference takes from heap
addresses are taken from the keys (docs/parity.md)."""


class Node:
    """The graph members of one KeyFrame."""

    def __init__(self):
        self.weights = {}        # mConnectedKeyFrameWeights
        self.ordered = []        # mvpOrderedConnectedKeyFrames
        self.ordered_w = []      # mvOrderedWeights
        self.first = True        # mbFirstConnection
        self.parent = None       # mpParent
        self.children = set()    # mspChildrens


class Graph:
    def __init__(self, root_key=1):
        self.nodes = {}
        self.root_key = root_key     # the key frame with mnId == 0: it never takes a parent

    def node(self, kf):
        return self.nodes.setdefault(kf, Node())


def counter(world, kf):
    """KFcounter as (kf_key, count) in ascending key order; [] is the reference's early return."""
    c = {}
    for key in world.kfs[kf]:                      # vpMP = mvpMapPoints
        if not key:
            continue
        mp = world.points.get(key)
        if mp is None or mp["bad"]:                # (a point the map forgot has no observations)
            continue
        for other in mp["obs"]:                    # observations = pMP->GetObservations()
            if other == kf:
                continue
            c[other] = c.get(other, 0) + 1
    return sorted(c.items())


def select(cnt, th):
    """vPairs before the sort: the links of weight >= th, or the first maximum in ascending key order."""
    nmax, kmax, pairs = 0, None, []
    for k, w in cnt:
        if w > nmax:
            nmax, kmax = w, k
        if w >= th:
            pairs.append((w, k))
    if not pairs and kmax is not None:
        pairs.append((nmax, kmax))
    return pairs


def ordered(pairs):
    """sort(vPairs) and push_front: descending weight, ties by descending key."""
    s = sorted(pairs)
    return [k for _, k in reversed(s)], [w for w, _ in reversed(s)]


def update_best_covisibles(node):
    """Every entry of mConnectedKeyFrameWeights, the ones below the threshold included."""
    node.ordered, node.ordered_w = ordered([(w, k) for k, w in node.weights.items()])


def add_connection(graph, kf, other, weight):
    n = graph.node(kf)
    if other in n.weights and n.weights[other] == weight:
        return
    n.weights[other] = weight
    update_best_covisibles(n)


def update_connections(world, graph, kf, th=15):
    cnt = counter(world, kf)
    if not cnt:
        return
    pairs = select(cnt, th)
    for w, k in pairs:
        add_connection(graph, k, kf, w)
    n = graph.node(kf)
    n.weights = dict(cnt)
    n.ordered, n.ordered_w = ordered(pairs)
    if n.first and kf != graph.root_key:
        n.parent = n.ordered[0]
        graph.node(n.parent).children.add(kf)
        n.first = False


def covis(world, kf_keys, th=15):
    """What orbhip_map_covis returns through orbhip.localmap.LocalMap.covis: (keys, weights, ordered keys) per query."""
    out = []
    for kf in kf_keys:
        cnt = counter(world, int(kf))
        out.append(([k for k, _ in cnt], [w for _, w in cnt], ordered(select(cnt, th))[0]))
    return out


def brute_weights(world, kf):
    """w(kf, j) by set intersection of the rows' good points: the cross-check of counter()."""
    good = lambda row: set(k for k in row if k and k in world.points and not world.points[k]["bad"])
    mine = good(world.kfs[kf])
    out = []
    for j in sorted(world.kfs):
        if j != kf:
            n = len(mine & good(world.kfs[j]))
            if n:
                out.append((j, n))
    return out
