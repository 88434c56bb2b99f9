"""Inputs of the loop-closure front-end tests: crops of tests/golden/mh04_frames.npz (through pt_inputs), a few synthetic planes,
and the BRIEF pattern of the reference's settings file (tests/golden/brief_pattern.npz).  References are computed once per
process and shared (lru_cache); callers do not modify them."""
import functools
import os

import numpy as np

import lc_ref
import pt_inputs
import pt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = pt_ref.EUROC_CAM0
FAST_TH = 20          # keyframe.cpp:90


@functools.lru_cache(maxsize=None)
def pattern():
    f = np.load(os.path.join(ROOT, "tests", "golden", "brief_pattern.npz"))
    p = tuple(np.ascontiguousarray(f[k], np.int32) for k in ("x1", "y1", "x2", "y2"))
    assert all(a.shape == (256,) for a in p)
    for a in p:
        a.setflags(write=False)
    return p


def constant(w, h, value=93):
    return np.full((h, w), value, np.uint8)


@functools.lru_cache(maxsize=None)
def image_cases():
    """name -> images [n][H][W]: the cases of the blur plane and the FAST list"""
    c = pt_inputs.crop
    rng = np.random.RandomState(7)
    seven = rng.randint(0, 256, (7, 7)).astype(np.uint8)
    seven[3, 3] = 128
    for dx, dy in lc_ref.CIRCLE[:10]:          # ten contiguous bright circle pixels: the one candidate pixel is a corner
        seven[3 + dy, 3 + dx] = 250
    for dx, dy in lc_ref.CIRCLE[10:]:
        seven[3 + dy, 3 + dx] = 120
    return {
        "crop160x120": c(3, 300, 200, 160, 120)[None],
        "crop75x53": c(4, 410, 215, 75, 53)[None],
        "7x7": seven[None],
        "constant": constant(64, 48)[None],
        "batch3_constant_in_the_middle": np.stack([c(5, 100, 100, 160, 120), constant(160, 120), c(6, 420, 250, 160, 120)]),
    }


def corner_blob(img, x, y, centre, ring):
    """paints a FAST corner at (x, y): the centre pixel and all 16 circle pixels (score = |centre - ring| - 1)"""
    img[y, x] = centre
    for dx, dy in lc_ref.CIRCLE:
        img[y + dy, x + dx] = ring


BORDER_CORNERS = ((3, 14), (36, 14), (20, 3), (20, 26), (3, 3), (36, 26))
TIE = ((18, 11), (19, 11))


@functools.lru_cache(maxsize=None)
def ties_and_borders():
    """a 40 x 30 plane of 100 with full-ring corners (score 59) at distance 3 from each border and from two image corners
    (BORDER_CORNERS), and a bright bar whose right end makes (18, 11) and (19, 11) ADJACENT corners of equal score 79 (TIE): with
    the strict comparison neither survives"""
    W, H = 40, 30
    img = np.full((H, W), 100, np.uint8)
    for x, y in BORDER_CORNERS:
        corner_blob(img, x, y, 100, 160)
    img[10:14, 6:20] = 180
    img.setflags(write=False)
    return img


def brief_border_points(W, H):
    """fractional window points within 24 pixels of every border and corner, points whose sum with a pattern offset falls in
    (-1, 0), one point outside the image and one far outside"""
    x1, y1, x2, y2 = pattern()
    pts = []
    for x in (0.25, 5.5, 23.75, W / 2 + 0.5, W - 24.25, W - 6.5, W - 1.0, W - 0.25):
        for y in (0.75, 7.25, 23.5, H / 2 + 0.25, H - 23.75, H - 5.5, H - 1.0, H - 0.5):
            pts.append((x, y))
    # pt + offset in (-1, 0): truncation puts the test on column / row 0
    neg = [int(v) for v in np.unique(np.concatenate([x1, y1, x2, y2])) if v < 0][:6]
    for o in neg:
        pts.append((-o - 0.5, H / 2.0))
        pts.append((W / 2.0, -o - 0.25))
    pts.append((-40.0, -40.0))            # every test outside: all bits 0
    pts.append((W + 100.5, H / 2.0))
    pts.append((1.0e12, 3.0))             # beyond the range of the conversion: outside
    return np.asarray(pts, np.float32)


@functools.lru_cache(maxsize=None)
def ref_keyframe(case):
    """per image of the case: (blurred, keypoints, scores, score plane, keypoints_norm, brief)"""
    out = []
    for img in image_cases()[case]:
        b = lc_ref.blur(img)
        kp, sc, plane = lc_ref.fast(img, FAST_TH)
        out.append((b, kp, sc, plane, lc_ref.lift(CAM, kp), lc_ref.brief(b, kp, pattern())))
    return out


@functools.lru_cache(maxsize=None)
def displaced_pair(ox=5, oy=-3, w=200, h=150):
    """two crops of one frame whose content moves by (ox, oy): (a, b)"""
    return pt_inputs.crop(1, 260, 160, w, h), pt_inputs.crop(1, 260 - ox, 160 - oy, w, h)


def descriptor_with_distance(base, dist, rng):
    """a copy of the [4] uint64 descriptor with exactly `dist` bits flipped"""
    bits = lc_ref.unpack_bits(base)[0].copy()
    flip = rng.choice(256, dist, replace=False)
    bits[flip] = ~bits[flip]
    return lc_ref.pack_bits(bits[None])[0]


@functools.lru_cache(maxsize=None)
def synthetic_match_pairs(tile=1024):
    """list of (window_brief [k][4], old_brief [m][4], old_kp [m][2], old_norm [m][2]) with the distances the rules turn on"""
    rng = np.random.RandomState(11)

    def rand_desc(n):
        return lc_ref.pack_bits(rng.randint(0, 2, (n, 256)).astype(bool)).reshape(n, 4)

    def kps(m):
        kp = rng.uniform(0, 700, (m, 2)).astype(np.float32)
        return kp, ((kp - 350) / 460).astype(np.float32)

    pairs = []
    # pairs 0 .. 6 (RULE_PAIRS): one window descriptor each and old descriptors at exact distances from it
    def rule(dists, duplicate_of=None):
        w = rand_desc(1)
        old = [descriptor_with_distance(w[0], d, rng) for d in dists]
        if duplicate_of is not None:
            old.append(old[duplicate_of].copy())
        pairs.append((w, np.asarray(old, np.uint64)) + kps(len(old)))

    rule([200, 79, 200])              # 79: accepted, index 1
    rule([80, 130])                   # 80: the best, refused
    rule([127])                       # 127: the best, refused
    rule([128, 200])                  # nothing below 128: no index
    rule([41, 40, 44], duplicate_of=1)  # a duplicate of the best: the lower index, 1
    rule([90, 33, 33, 33])            # a tie of different descriptors: the lowest index, 1
    rule([5, 0, 0])                   # distance 0, twice
    # pair 7: an old list longer than one LDS tile; the best of window 0 lies in the second tile, window 1 ties across the tiles
    m = tile + 300
    win = rand_desc(5)
    old = np.stack([descriptor_with_distance(win[i % 5], 140 + (i % 17), rng) for i in range(m)])
    old[tile + 17] = descriptor_with_distance(win[0], 12, rng)
    old[5] = descriptor_with_distance(win[1], 30, rng)
    old[tile + 5] = descriptor_with_distance(win[1], 30, rng)
    old[tile - 1] = descriptor_with_distance(win[2], 60, rng)
    old[tile] = descriptor_with_distance(win[2], 59, rng)
    pairs.append((win, old) + kps(m))
    # pair 8: an empty old list;  pair 9: an empty window list;  pair 10: 150 random against 333 random
    pairs.append((rand_desc(4), np.zeros((0, 4), np.uint64)) + kps(0))
    pairs.append((np.zeros((0, 4), np.uint64), rand_desc(9)) + kps(9))
    pairs.append((rand_desc(150), rand_desc(333)) + kps(333))
    return pairs


def walsh_desc(k):
    """descriptor k = 0 .. 254 of a family whose members differ pairwise in exactly 128 bits: bit b = parity of b & (k + 1)"""
    b = np.arange(256)
    return lc_ref.pack_bits(np.array([bin(int(v) & (k + 1)).count("1") & 1 for v in b], bool)[None])[0]


@functools.lru_cache(maxsize=None)
def glue_pair():
    """six window descriptors exactly 128 bits apart and four old ones 30 bits from window 0, 40 and 20 from window 3 and 0 from
    window 5: every other distance is at least 128 - 40, so the status is 1 0 0 1 0 1 and the matched old indices are 0, 2, 3
    -> (window_brief, old_brief, old_kp, old_norm)"""
    rng = np.random.RandomState(5)
    win = np.stack([walsh_desc(k) for k in range(6)])
    old = np.stack([descriptor_with_distance(win[0], 30, rng), descriptor_with_distance(win[3], 40, rng),
                    descriptor_with_distance(win[3], 20, rng), win[5].copy()])
    kp = rng.uniform(0, 700, (4, 2)).astype(np.float32)
    return win, old, kp, ((kp - 350) / 460).astype(np.float32)


# ---- loop verification: scenes built as pt_inputs.rigid_scene is: a pose, points in front of it, their normalised projections ----
def _rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


QIC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # camera z forwards along the body's x, x to the right
TIC = np.array([0.05, -0.02, 0.01])
LOOP_NOISE, LOOP_OUTLIER = 1e-3, 0.1         # inliers at most 1e-3 from their projection, outliers at least 0.1 (threshold 0.0217)


@functools.lru_cache(maxsize=None)
def loop_scene(n, n_outliers, rng_seed, yaw_deg=8.0, shift=(0.6, -0.4, 0.1), depth=(4.0, 12.0)):
    """The current keyframe at a body pose of its own, the old one turned by yaw_deg about the world's z and moved by `shift`
    from it; n world points in front of both cameras, rounded to float; their projections into the OLD camera displaced by at most
    LOOP_NOISE, the first n_outliers by LOOP_OUTLIER .. 0.5 instead; the list shuffled.
    -> dict pts3d [n][3], old_norm [n][2] float32, outlier [n] bool, origin_vio_T, origin_vio_R, old_T, old_R"""
    rng = np.random.RandomState(rng_seed)
    vio_R = _rot_z(20.0) @ np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]])
    vio_T = np.array([2.0, -1.0, 0.5])
    old_R = _rot_z(yaw_deg) @ vio_R
    old_T = vio_T + np.asarray(shift, np.float64)
    Rc, Tc = vio_R @ QIC, vio_T + vio_R @ TIC
    Ro, To = old_R @ QIC, old_T + old_R @ TIC
    pts = np.zeros((0, 3))
    while len(pts) < n:
        m = 8 * n
        z = rng.uniform(depth[0], depth[1], m)
        pc = np.stack([rng.uniform(-0.6, 0.6, m) * z, rng.uniform(-0.4, 0.4, m) * z, z], axis=1)      # in the current camera
        pw = (pc @ Rc.T + Tc).astype(np.float32).astype(np.float64)
        po = (pw - To) @ Ro
        ok = (po[:, 2] > 1.0) & (np.abs(po[:, 0] / po[:, 2]) < 1.2) & (np.abs(po[:, 1] / po[:, 2]) < 0.8)
        pts = np.concatenate([pts, pw[ok]])
    pts = pts[:n]
    po = (pts - To) @ Ro
    uv = po[:, :2] / po[:, 2:3]
    r, a = LOOP_NOISE * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    r[:n_outliers] = rng.uniform(LOOP_OUTLIER, 0.5, n_outliers)
    uv = uv + np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
    outlier = np.zeros(n, bool)
    outlier[:n_outliers] = True
    perm = rng.permutation(n)
    return dict(pts3d=pts[perm].astype(np.float32), old_norm=uv[perm].astype(np.float32), outlier=outlier[perm],
                origin_vio_T=vio_T, origin_vio_R=vio_R, old_T=old_T, old_R=old_R)


LOOP_CASES = {
    "40 points, no outliers": dict(scene=(40, 0, 1), seed=101, stage=lc_ref.CLOSED),
    "60 points, 30 % outliers": dict(scene=(60, 18, 2), seed=102, stage=lc_ref.CLOSED),
    "26 points, all inliers": dict(scene=(26, 0, 3), seed=103, stage=lc_ref.CLOSED),
    "25 points": dict(scene=(25, 0, 4), seed=104, stage=lc_ref.FEW_POINTS),
    "40 points, 25 inliers": dict(scene=(40, 15, 5), seed=105, stage=lc_ref.FEW_INLIERS),
    "relative yaw 35 degrees": dict(scene=(40, 0, 6, 35.0), seed=106, stage=lc_ref.REJECTED),
    "relative translation 25 m": dict(scene=(40, 0, 7, 5.0, (15.0, -20.0, 0.0), (40.0, 90.0)), seed=107, stage=lc_ref.REJECTED),
}


def loop_case(name):
    """-> (scene dict, seed)"""
    c = LOOP_CASES[name]
    return loop_scene(*c["scene"]), c["seed"]


@functools.lru_cache(maxsize=None)
def ref_loop_case(name):
    """(float64 run, extended-precision run) of lc_ref.verify"""
    S, seed = loop_case(name)
    return tuple(lc_ref.verify(S["pts3d"], S["old_norm"], S["origin_vio_T"], S["origin_vio_R"], TIC, QIC, seed, dt)
                 for dt in (np.float64, np.longdouble))
