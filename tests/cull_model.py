"""Independent model of LocalMapping::KeyFrameCulling's counting loop (ref: src/LocalMapping.cc:2705-2753; the fork's
KeyFrameCullingForMonoVI has the same loop at :1533-1581), written on the observation maps of tests/localmap_collect_model.py's
World plus one level byte per (key frame, feature index): for every point of the candidate the walk goes over the point's own
key frame -> index map and compares octaves, with the reference's break.  It does not count by octave and does not walk rows of
other key frames: that is the formulation of the kernels under test.  Keys stand for pointers; 0 is NULL."""

OCTAVE, STEREO, FAR = 0x0F, 0x40, 0x80


def level_byte(octave, stereo=False, far=False):
    assert 0 <= octave <= 15
    return octave | (STEREO if stereo else 0) | (FAR if far else 0)


class Levels:
    """mvKeysUn[i].octave, mvuRight[i] >= 0 and "mvDepth[i] > mThDepth || mvDepth[i] < 0" of every key frame's features."""

    def __init__(self):
        self.rows = {}           # kf -> list of level bytes

    def put(self, kf, row):
        self.rows[kf] = [int(b) for b in row]

    def octave(self, kf, idx):
        return self.rows[kf][idx] & OCTAVE

    def stereo(self, kf, idx):
        return bool(self.rows[kf][idx] & STEREO)

    def far(self, kf, idx):
        return bool(self.rows[kf][idx] & FAR)


def observations(levels, mp):
    """MapPoint::Observations(): nObs as AddObservation / EraseObservation keep it, +2 for a stereo observation."""
    return sum(2 if levels.stereo(kf, idx) else 1 for kf, idx in mp["obs"].items())


def count(world, levels, kf, monocular, th_obs=3):
    """(nMPs, nRedundantObservations, entry states) of one candidate; state 0 not counted, 1 counted, 2 counted and redundant."""
    n_mps = n_red = 0
    states = []
    for i, key in enumerate(world.kfs[kf]):            # vpMapPoints = pKF->GetMapPointMatches()
        states.append(0)
        if not key:
            continue
        mp = world.points.get(key)
        if mp is None or mp["bad"]:
            continue
        if not monocular:
            if levels.far(kf, i):
                continue
        n_mps += 1
        states[i] = 1
        if observations(levels, mp) > th_obs:
            scale_level = levels.octave(kf, i)
            n_obs = 0
            for kfi, idx in mp["obs"].items():
                if kfi == kf:
                    continue
                if levels.octave(kfi, idx) <= scale_level + 1:
                    n_obs += 1
                    if n_obs >= th_obs:
                        break
            if n_obs >= th_obs:
                n_red += 1
                states[i] = 2
    return n_mps, n_red, states


def is_redundant(n_mps, n_red):
    return float(n_red) > 0.9 * float(n_mps)             # nRedundantObservations>0.9*nMPs, in double


def cull(world, levels, kf_keys, monocular, th_obs=3):
    """What orbhip_map_cull returns: counts, redundant and entry states of every candidate on the map as it is."""
    counts, red, states = [], [], []
    for kf in kf_keys:
        m, r, s = count(world, levels, int(kf), monocular, th_obs)
        counts.append((m, r))
        red.append(is_redundant(m, r))
        states.append(s)
    return counts, red, states


def erase_observation(world, levels, key, kf):
    """MapPoint::EraseObservation: the count goes down by 1 or 2; at nObs <= 2 SetBadFlag erases the point from its observers."""
    mp = world.points[key]
    if kf in mp["obs"]:
        levels_before = observations(levels, mp)
        idx = mp["obs"].pop(kf)                                    # (the culled key frame keeps its mvpMapPoints)
        assert observations(levels, mp) == levels_before - (2 if levels.stereo(kf, idx) else 1)
        if observations(levels, mp) <= 2:
            mp["bad"] = True
            for kfi, i in mp["obs"].items():                       # SetBadFlag: EraseMapPointMatch in every observer
                world.kfs[kfi][i] = 0
            mp["obs"] = {}


def set_bad_flag(world, levels, kf):
    """The observation half of KeyFrame::SetBadFlag; the key frame then leaves the map."""
    for key in list(world.kfs[kf]):
        if key and key in world.points:
            erase_observation(world, levels, key, kf)
    del world.kfs[kf]


def sequential(world, levels, kf_keys, monocular, skip=lambda kf: False, root_key=1, th_obs=3):
    """The loop of KeyFrameCulling over vpLocalKeyFrames = kf_keys, editing the world between candidates.  skip(kf) is asked at
    the candidate's turn.  Returns the culled key frames in order."""
    culled = []
    for kf in kf_keys:
        kf = int(kf)
        if kf == root_key:                               # pKF->mnId==0
            continue
        if skip(kf):
            continue
        m, r, _ = count(world, levels, kf, monocular, th_obs)
        if is_redundant(m, r):
            set_bad_flag(world, levels, kf)
            culled.append(kf)
    return culled


# ---- the two scenes that say why a batch is not the sequence (tests/test_cull_model.py, tests/native_cull/test_cull.cpp) ----
def scene_a():
    """A, B, C, D all see P1..P10 at octave 0, monocular.  Candidates A then B.  At the start both are redundant (obs 4, others 3).
    Culling A leaves obs 3, which is not > 3: B stays."""
    import localmap_collect_model as CM
    w, lv = CM.World(), Levels()
    pts = list(range(1, 11))
    for p in pts:
        w.add_point(p)
    for kf in (2, 3, 4, 5):                               # A = 2, B = 3, C = 4, D = 5 (1 is the key frame with mnId 0)
        w.put_kf(kf, pts)
        lv.put(kf, [level_byte(0)] * 10)
    return w, lv, [2, 3]


def scene_b():
    """A sees S1..S20 (with C, D, E) and W1, W2 (with B and F alone); B sees Q1..Q10 (with C, D, E) and W1, W2.  At the start A is
    redundant (20 of 22) and B is not (10 of 12).  Culling A leaves W1, W2 with two observers: they turn bad, B counts 10 of 10."""
    import localmap_collect_model as CM
    w, lv = CM.World(), Levels()
    S, Q, W = list(range(1, 21)), list(range(21, 31)), [31, 32]
    for p in S + Q + W:
        w.add_point(p)
    rows = {2: S + W, 3: Q + W, 4: S + Q, 5: S + Q, 6: S + Q, 7: W}   # A = 2, B = 3, C, D, E = 4, 5, 6, F = 7
    for kf, row in rows.items():
        w.put_kf(kf, row)
        lv.put(kf, [level_byte(0)] * len(row))
    return w, lv, [2, 3]
