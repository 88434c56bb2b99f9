"""Inputs of the point front-end tests, all drawn from tests/golden/mh04_frames.npz (15 consecutive 752 x 480 EuRoC frames)
and crops of them.  The reference results are computed once per process and shared (lru_cache); callers do not modify them."""
import functools
import os

import numpy as np

import pt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CNT, MIN_DIST = 150, 30     # euroc_config.yaml: max_cnt, min_dist


@functools.lru_cache(maxsize=None)
def frames():
    f = np.load(os.path.join(ROOT, "tests", "golden", "mh04_frames.npz"))["frames"]
    assert f.shape == (15, 480, 752) and f.dtype == np.uint8
    f.setflags(write=False)
    return f


def crop(frame, x0, y0, w, h):
    return np.ascontiguousarray(frames()[frame][y0:y0 + h, x0:x0 + w])


def disc_mask_40(H=480, W=752):
    """setMask's plane after 40 kept points: discs of radius MIN_DIST around the first 40 corners of frame 1's detection"""
    c, _ = ref_detect_full(1)
    return pt_ref.disc_mask(H, W, [(int(x), int(y)) for x, y in c[:40]], MIN_DIST)


def sparse_mask_64x48():
    """a plane that leaves two 7 x 7 windows of a 64 x 48 crop open: fewer candidates than max_corners"""
    m = np.zeros((48, 64), np.uint8)
    m[8:15, 10:17] = 255
    m[30:37, 40:47] = 1        # any non-zero value allows
    return m


@functools.lru_cache(maxsize=None)
def ref_detect_full(frame):
    """the reference detector on a full golden frame, max_corners 150, min_distance 30, no mask"""
    return pt_ref.detect(frames()[frame], MAX_CNT, MIN_DIST)


@functools.lru_cache(maxsize=None)
def detect_cases():
    """name -> (images [n][H][W], max_corners [n], min_distance [n], masks or None): the five cases of the detector"""
    f = frames()
    const = np.full((120, 160), 93, np.uint8)
    return {
        "full": (f[1:2], [150], [30.0], None),
        "full_mask40": (f[2:3], [37], [30.0], [disc_mask_40()]),
        "crop160x120": (crop(3, 300, 200, 160, 120)[None], [150], [10.0], None),
        "crop64x48_sparse_mask": (crop(4, 400, 220, 64, 48)[None], [50], [3.0], [sparse_mask_64x48()]),
        "batch3_one_constant": (np.stack([crop(5, 100, 100, 160, 120), const, crop(6, 420, 250, 160, 120)]), [40, 40, 25],
                                [8.0, 8.0, 12.5], None),
    }


@functools.lru_cache(maxsize=None)
def ref_detect_case(name):
    images, mc, md, masks = detect_cases()[name]
    return [pt_ref.detect(images[i], mc[i], md[i], None if masks is None else masks[i], return_total=True) for i in range(len(images))]


# ---- rejectWithF: correspondences of a synthetic rigid scene through the distorted pinhole ----------------------------------
CAM = pt_ref.EUROC_CAM0
W, H = 752, 480


@functools.lru_cache(maxsize=None)
def rigid_scene(n, n_outliers, rng_seed):
    """n points 3 .. 9 m in front of camera 1, seen again from a camera moved 12 cm sideways, 3 cm forwards and turned by two
    degrees; both views through the distorted EuRoC model, rounded to float as a tracker holds them.  The first n_outliers of
    the second view are displaced by 5 .. 20 px up or down: the camera moves and turns in its x-z plane, so the epipolar lines
    run within a few degrees of the image rows and a vertical displacement of 5 px leaves the line by well over F_THRESHOLD = 1 px
    (a displacement ALONG the line is invisible to any fundamental matrix).  The list is shuffled.
    -> (cur [n][2], forw [n][2] float32, outlier [n] bool)"""
    rng = np.random.RandomState(rng_seed)
    cur = np.zeros((0, 2))
    forw = np.zeros((0, 2))
    while len(cur) < n:
        m = 4 * n
        u, v = rng.uniform(20, W - 20, m), rng.uniform(20, H - 20, m)
        x, y = pt_ref.lift_projective(CAM, u, v)
        z = rng.uniform(3.0, 9.0, m)
        P = np.stack([x * z, y * z, z], axis=1)
        a = np.deg2rad(2.0)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Q = (P - np.array([0.12, 0.0, 0.03])) @ R
        u2, v2 = pt_ref.space_to_plane(CAM, Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2])
        ok = (u2 > 20) & (u2 < W - 20) & (v2 > 20) & (v2 < H - 20)
        cur = np.concatenate([cur, np.stack([u, v], axis=1)[ok]])
        forw = np.concatenate([forw, np.stack([u2, v2], axis=1)[ok]])
    cur, forw = cur[:n].copy(), forw[:n].copy()
    outlier = np.zeros(n, bool)
    outlier[:n_outliers] = True
    forw[:n_outliers, 1] += rng.uniform(5.0, 20.0, n_outliers) * rng.choice([-1.0, 1.0], n_outliers)
    perm = rng.permutation(n)
    return cur[perm].astype(np.float32), forw[perm].astype(np.float32), outlier[perm]


def reject_cases():
    """name -> list of (cur, forw, seed): 7 points, 8 points, 150 with a fifth outliers, a batch of two with different seeds"""
    c7, f7, _ = rigid_scene(7, 0, 1)
    c8, f8, _ = rigid_scene(8, 0, 2)
    c150, f150, _ = rigid_scene(150, 30, 3)
    c90, f90, _ = rigid_scene(90, 18, 4)
    return {"7_points": [(c7, f7, 11)], "8_points": [(c8, f8, 12)], "150_points_30_outliers": [(c150, f150, 13)],
            "batch_of_2": [(c150, f150, 14), (c90, f90, 15)]}


# ---- calcOpticalFlowPyrLK -------------------------------------------------------------------------------------------------
def displaced_crops(ox, oy, x0=200, y0=120, w=320, h=240, frame=1):
    """two crops of one frame whose content moves by (ox, oy) whole pixels from the first to the second, and the reference
    detector's corners of the first whose 21 x 21 window stays inside both crops"""
    a, b = crop(frame, x0, y0, w, h), crop(frame, x0 - ox, y0 - oy, w, h)
    c, _ = pt_ref.detect(a, 150, 12.0)
    inside = ((c[:, 0] - 10 + min(ox, 0) >= 0) & (c[:, 0] + 10 + max(ox, 0) < w) &
              (c[:, 1] - 10 + min(oy, 0) >= 0) & (c[:, 1] + 10 + max(oy, 0) < h))
    return a, b, c[inside]


@functools.lru_cache(maxsize=None)
def flow_cases():
    """name -> (images [n][H][W], pairs [(prev, next)], prev_pts per pair): the five cases of the tracker"""
    f = frames()
    full_pts, _ = ref_detect_full(1)
    ca, cb = crop(1, 300, 200, 160, 120), crop(2, 300, 200, 160, 120)
    crop_pts, _ = pt_ref.detect(ca, 40, 8.0)
    W_, H_ = 752, 480
    border_pts = np.array([(5, 5), (W_ - 6, 5), (5, H_ - 6), (W_ - 6, H_ - 6), (376, 3), (376, H_ - 4), (3, 240), (W_ - 4, 240),
                           (11.5, 11.25), (W_ - 12.5, H_ - 11.75), (0.5, 0.5), (W_ - 1, H_ - 1),
                           (-11.5, 200.0),            # its window starts left of the 21-pixel border: status 0
                           (W_ + 9.5, 100.0)], np.float32)   # right of the image: status 0
    pa, pb = ca.copy(), cb.copy()
    pa[30:90, 40:110] = 128
    pb[30:90, 40:110] = 128
    flat_pts = np.array([(75, 60), (60.5, 55.25), (20, 20), (130, 100)], np.float32)   # two in the constant patch, two outside
    c4 = [crop(k, 300, 200, 160, 120) for k in (3, 4, 5, 6)]
    p65, _ = pt_ref.detect(c4[2], 65, 4.0)
    assert len(p65) == 65
    p1, _ = pt_ref.detect(c4[1], 1, 4.0)
    return {
        "frames_1_2_150_points": (f[1:3], [(0, 1)], [full_pts]),
        "crop160x120_3_levels": (np.stack([ca, cb]), [(0, 1)], [crop_pts]),
        "borders_and_corners": (f[1:3], [(0, 1)], [border_pts]),
        "constant_patch": (np.stack([pa, pb]), [(0, 1)], [flat_pts]),
        "batch_0_1_65_points": (np.stack(c4), [(0, 1), (1, 2), (2, 3)], [np.zeros((0, 2), np.float32), p1, p65]),
    }


@functools.lru_cache(maxsize=None)
def ref_flow_case(name):
    images, pairs, pts = flow_cases()[name]
    return [pt_ref.lk_flow(images[a], images[b], p) for (a, b), p in zip(pairs, pts)]
