"""Stereo pairs for the ComputeStereoMatches tests (tests/test_stereo.py): natural scenes whose right image is a
resampling of the left one (fractional, slanted disparity; vertical offset; gain and noise), and hand-built pairs
with planted keypoints whose answers are known.

Planting relies on the C ABI taking any keypoint arrays and reading pixels from the pyramids the two contexts last
extracted: extract the images first, then append keypoints and descriptors.

Precondition of every planted keypoint that reaches the GPU: 0 <= octave < nlevels and at least 16 px inside the
image at its own octave, as extractor keypoints are.  k_stereo_refine loads its patches on that assumption
(csrc/k_stereo.hip, the patch loads in k_stereo_refine), and the reference is undefined outside it.

The border skip (iniu < 0 || endu >= cols, src/Frame.cc:921-923) cannot be reached under that rule.  A right
keypoint of octave o lies at x <= (W_o - 17) * s^o.  Its column at the left octave o - 1 is
round(x / s^(o-1)) <= round((W_o - 17) * s) ~= W_(o-1) - 20.4, and at octave o + 1 it is about W_(o+1) - 14.2
(widths round, so allow a pixel).  endu = scaleduR0 + 11 >= W needs scaleduR0 >= W - 11, so no extractor-like
keypoint gets there; on the left, scaleduR0 >= 16 / 1.2 - 1 > 0 likewise.  That branch is therefore tested only
in the CPU model and the oracle, and only at the right edge or with scaleduR0 < 0: with 0 <= scaleduR0 < 10 the
reference's check lets the keypoint through and then reads left of the image.
"""
import numpy as np

from orbhip import synth

KITTI = (1241, 376, 2000, 0.54, 386.1)     # width, height, features, mb, mbf (KITTI00-02.yaml)
EUROC = (752, 480, 1200, 0.11, 47.9)       # EuRoC stereo

# right(x, y) = src(x + PADX + d(x, y), y + PADY + dy), left(x, y) = src(x + PADX, y + PADY): a point at uL is seen at
# uL - d, one row band dy higher.  d(x, y) = d0 + ax * x / W + ay * y / H.
PADX, PADY = 16, 8
KINDS = {
    "shift": dict(d=(17.0, 0.0, 0.0), dy=0.0),                                  # integer disparity, like make_stereo_pair
    "slant04": dict(d=(9.3, 6.7, 3.1), dy=0.4),
    "slant13": dict(d=(21.7, -8.9, 5.3), dy=1.3),
    "slant25": dict(d=(5.45, 4.4, 0.0), dy=2.5),                                # outside the octave-0 band, inside higher ones
    "gain": dict(d=(13.2, 3.8, 4.1), dy=0.4, gain=1.3, sigma=8.0),              # patch distances in the thousands
    "maxd": dict(d=(28.0, 24.0, 0.0), dy=0.0, baseline=(0.5, 20.0)),            # maxD = 40 crossed at x = W / 2
    "photo": dict(d=(11.4, 5.2, 2.6), dy=1.3, gain=1.3, sigma=8.0, photo=True),
}


def kinds():
    """The scene kinds this machine can make ("photo" needs the sample photographs)."""
    return [k for k in KINDS if k != "photo" or synth.load_photographs()]


def mirror_patch(rng, h=15, w=31):
    """A random patch symmetric about its centre column: around its centre, the patch distance of shift +s equals
    that of shift -s."""
    half = rng.integers(60, 190, (h, w // 2 + 1)).astype(np.uint8)
    return np.concatenate([half[:, :0:-1], half], axis=1)


def paste(img, patch, cx, cy):
    h, w = patch.shape
    img[cy - h // 2:cy + h // 2 + 1, cx - w // 2:cx + w // 2 + 1] = patch


def perturb(img, cx, cy, k):
    """Add k to the 11x11 patch distance at (cx, cy) of img against an unchanged copy, keeping img symmetric about
    column cx: equal increments at (cy + dy, cx +- dx), the odd unit on the centre column; the centre stays."""
    left = k
    for dy in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5):
        for dx in range(1, 6):
            q = min(left // 2, 40)
            img[cy + dy, cx - dx] += q
            img[cy + dy, cx + dx] += q
            left -= 2 * q
    img[cy + 1, cx] += left
    assert left <= 40


def scene(kind, seed, W, H, mb, mbf, nplant=4):
    """(left, right, plants, mb, mbf): a natural pair of `kind` with `nplant` mirror patches pasted at the same place in
    both images (disparity 0, for plant_zero())."""
    p = KINDS[kind]
    mb, mbf = p.get("baseline", (mb, mbf))
    rng = np.random.default_rng(1000 * seed + sorted(KINDS).index(kind))
    SW, SH = W + PADX + 96, H + 2 * PADY + 8
    if p.get("photo"):
        src = synth.photograph_frames(SW, SH, 1 + seed % 3)[-1]
    else:
        src = synth.warp_frame(synth.make_scene(seed, SW, SH), SW, SH, 0)
    left = src[PADY:PADY + H, PADX:PADX + W].copy()
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    d0, ax, ay = p["d"]
    mapx = (xx + np.float32(PADX) + np.float32(d0) + np.float32(ax / W) * xx + np.float32(ay / H) * yy).astype(np.float32)
    mapy = (yy + np.float32(PADY + p["dy"])).astype(np.float32)
    import orb_oracle_py as oracle
    right = oracle.remap_linear(src, mapx, mapy)
    if "gain" in p:
        right = np.clip(np.rint(p["gain"] * right.astype(np.float64) + rng.normal(0, p["sigma"], right.shape)), 0,
                        255).astype(np.uint8)
    plants = []
    for i in range(nplant):
        x0, x1 = (W * (i % 2)) // 2, (W * (i % 2 + 1)) // 2
        y0, y1 = (H * (i // 2 % 2)) // 2, (H * (i // 2 % 2 + 1)) // 2
        cx, cy = int(rng.integers(max(x0, 40), min(x1, W - 40))), int(rng.integers(max(y0, 30), min(y1, H - 30)))
        patch = mirror_patch(rng)
        paste(left, patch, cx, cy)
        paste(right, patch, cx, cy)
        plants.append((cx, cy))
    return left, right, plants, mb, mbf


def keypoint(x, y, octave=0):
    import orb_oracle_py as oracle
    k = np.zeros(1, oracle.KP_DTYPE)
    k["x"], k["y"], k["size"], k["octave"], k["class_id"] = x, y, 31.0, octave, -1
    return k


def plant_zero(kL, dL, kR, dR, plants, seed):
    """Append one octave-0 keypoint per mirror patch to both sides, with equal descriptors: distance 0, the patch
    distances of shifts -1 and +1 are equal, so deltaR = 0 and the disparity is exactly 0 (src/Frame.cc:955-958)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (len(plants), 32)).astype(np.uint8)
    kp = np.concatenate([keypoint(x, y) for x, y in plants]) if plants else kL[:0]
    return (np.concatenate([kL, kp]), np.concatenate([dL, d]), np.concatenate([kR, kp]), np.concatenate([dR, d]))


class Planted:
    """A hand-built pair: i.i.d. texture on both sides, and per slot a mirror patch seen at (px, py) on the left and
    (px - D, py) on the right, with one left keypoint at (px, py).  maxD = mbf / mb = maxd exactly (mb = 1).  Slots
    are 200 px and 25 rows apart, so no keypoint sees another slot's keypoints in its search range."""
    W, H = 640, 480

    def __init__(self, seed, maxd=24.0):
        self.rng = np.random.default_rng(seed)
        self.left = self.rng.integers(60, 190, (self.H, self.W)).astype(np.uint8)
        self.right = self.rng.integers(60, 190, (self.H, self.W)).astype(np.uint8)
        self.mb, self.mbf = 1.0, float(maxd)
        self.kL, self.dL, self.kR, self.dR = [], [], [], []
        self.want_u, self.want_z, self.avoid_u = [], [], []
        self.slots = [(px, py) for py in range(40, 441, 25) for px in (120, 320, 520)]

    def pair(self, D=1, sad=50, right=None, keep=True, slot=None):
        """One slot.  right: [(x, octave, hamming distance to the left descriptor)] in index order, default one
        keypoint on the patch with distance 5.  keep: True when the answer is the match at disparity D, False when it
        is no match, None when it is anything but the match at disparity D (want() gives NaN there and avoid() the
        value to miss).  Returns the left keypoint's index."""
        px, py = self.slots.pop(0) if slot is None else slot
        patch = mirror_patch(self.rng)
        paste(self.left, patch, px, py)
        r = patch.copy()
        perturb(r, 15, 7, sad)
        paste(self.right, r, px - D, py)
        desc = self.rng.integers(0, 256, 32).astype(np.uint8)
        for x, octave, ham in right if right is not None else [(px - D, 0, 5)]:
            dr = np.unpackbits(desc)
            dr[self.rng.choice(256, ham, replace=False)] ^= 1
            self.kR.append(keypoint(x, py, octave))
            self.dR.append(np.packbits(dr))
        self.kL.append(keypoint(px, py))
        self.dL.append(desc)
        f32 = np.float32
        self.avoid_u.append(f32(px - D) if D else f32(np.float64(f32(px)) - 0.01))
        if keep is None:
            self.want_u.append(f32(np.nan))
            self.want_z.append(f32(np.nan))
        elif not keep:
            self.want_u.append(f32(-1))
            self.want_z.append(f32(-1))
        elif D == 0:
            self.want_u.append(f32(np.float64(f32(px)) - 0.01))
            self.want_z.append(f32(self.mbf) / f32(0.01))
        else:
            self.want_u.append(f32(px - D))
            self.want_z.append(f32(self.mbf) / f32(D))
        return len(self.kL) - 1

    def lonely(self, x, y, xr=None, octave=0):
        """A left keypoint (and optionally a right one, distance 0) off the slot grid, on plain texture."""
        desc = self.rng.integers(0, 256, 32).astype(np.uint8)
        self.kL.append(keypoint(x, y, octave))
        self.dL.append(desc)
        if xr is not None:
            self.kR.append(keypoint(xr, y, octave))
            self.dR.append(desc.copy())
        self.want_u.append(np.float32(-1))
        self.want_z.append(np.float32(-1))
        self.avoid_u.append(np.float32(np.nan))
        return len(self.kL) - 1

    def arrays(self):
        import orb_oracle_py as oracle
        cat = lambda ks: np.concatenate(ks) if ks else np.zeros(0, oracle.KP_DTYPE)
        return (cat(self.kL), np.array(self.dL, np.uint8).reshape(-1, 32), cat(self.kR),
                np.array(self.dR, np.uint8).reshape(-1, 32))

    def want(self):
        return np.array(self.want_u, np.float32), np.array(self.want_z, np.float32)

    def avoid(self):
        return np.array(self.avoid_u, np.float32)
