"""Inputs of tests/test_triangulation_sets.py: key frame 1 and its neighbours from 320 x 240 synthetic stereo pairs, with the
k = 6, L = 4 synthetic vocabulary of tests/test_triangulation.py; the oracle's answers are computed once per configuration."""
import numpy as np

F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)      # pure horizontal translation: l = (0, 1, -y1)
F_GEN = np.array([[5e-7, 1e-5, -0.002], [-1e-5, 5e-7, -1.0], [0.0015, 1.0, 0.02]], np.float32)   # rows slightly rotated
F_GEN2 = np.array([[-2e-6, 1e-5, 0.002], [-1e-5, 2e-6, -1.0], [-0.001, 1.0, -0.03]], np.float32)

# (mono, only_stereo, check_ori): the four configurations of test_hip_search_for_triangulation_matches_oracle
CONFIGS = [(True, False, True), (False, False, True), (False, True, True), (True, False, False)]
SEED, NF, NF_SMALL = 8, 600, 120
# neighbour k: (disparity, F12, epipole); the last one is the small key frame
NEIGHBOURS = [(21, F_ROWS, (300.0, 240.0)), (19, F_GEN, (-80.0, 200.0)), (25, F_GEN2, (400.0, 120.0)), (21, F_ROWS, (150.0, 100.0))]
ANGLE_OFFSETS, ANGLE_P = np.array([0, 37, 75, 200], np.float32), [.55, .25, .15, .05]


def flags(n, seed, p):
    return (np.random.default_rng(seed).random(n) < p).astype(np.uint8)


def build(oracle):
    """{'kf1': (kps, desc, fv, skip, u_right), 'nb': [(kps, desc, fv, skip, u_right, F12, ex, ey)], 'sf', 's2'}.  Side-2 angles are
    turned by offsets drawn from ANGLE_OFFSETS so that the rotation histogram has something to remove."""
    from orbhip import distributed as D, synth
    voc = oracle.Vocabulary(D.make_synthetic_vocabulary(77, k=6, L=4))

    def features(img, nf):
        ex = oracle.Extractor(nf)
        k, d = ex(img)
        _, wt, nid = voc.transform(d, 2)
        return ex, k, d, oracle.feature_vector(nid, wt)

    left, _ = synth.make_stereo_pair(SEED, 320, 240, disparity=21)
    ex, k1, d1, g1 = features(left, NF)
    rng = np.random.default_rng(6)
    out = {"kf1": (k1, d1, g1, flags(len(k1), 4, 0.35), np.where(rng.random(len(k1)) < 0.6, k1["x"] - 20, -1).astype(np.float32)),
           "nb": [], "sf": np.array(list(ex.params.mvScaleFactor)[:8], np.float32),
           "s2": np.array(list(ex.params.mvLevelSigma2)[:8], np.float32)}
    for j, (disp, F, (exx, eyy)) in enumerate(NEIGHBOURS):
        _, right = synth.make_stereo_pair(SEED, 320, 240, disparity=disp)
        _, k2, d2, g2 = features(right, NF_SMALL if j == len(NEIGHBOURS) - 1 else NF)
        k2 = k2.copy()
        turn = np.random.default_rng(20 + j).choice(ANGLE_OFFSETS, len(k2), p=ANGLE_P).astype(np.float32)
        k2["angle"] = np.mod(k2["angle"] + turn, np.float32(360)).astype(np.float32)
        ur2 = np.where(np.random.default_rng(30 + j).random(len(k2)) < 0.6, k2["x"] - 20, -1).astype(np.float32)
        out["nb"].append((k2, d2, g2, flags(len(k2), 40 + j, 0.35), ur2, F, exx, eyy))
    return out


def oracle_rows(oracle, S, mono, only_stereo, check_ori):
    """[(nmatches, matches12)] per neighbour from the oracle."""
    k1, d1, g1, skip1, ur1 = S["kf1"]
    rows = []
    for k2, d2, g2, skip2, ur2, F, exx, eyy in S["nb"]:
        rows.append(oracle.search_for_triangulation(k1, d1, skip1, g1, k2, d2, skip2, g2, F, exx, eyy, S["sf"], S["s2"],
                                                    u_right1=None if mono else ur1, u_right2=None if mono else ur2,
                                                    only_stereo=only_stereo, check_ori=check_ori))
    return rows
