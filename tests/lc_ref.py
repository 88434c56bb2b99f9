"""NumPy restatement of the loop-closure front-end (csrc/lc_kernels.h), integer for integer: the 9 x 9, sigma 2 Gaussian blur of
DVision::BRIEF::compute, FAST 9-16 with score and non-maximum suppression, the BRIEF descriptor and the brute-force Hamming
search of KeyFrame::searchByBRIEFDes.  The blur's float arithmetic and FAST's score and list order are the ones lc_kernels.h
states from OpenCV's description; neither side is pinned by a run of OpenCV."""
import numpy as np

import pt_ref

F32 = np.float32
BLUR_R, BLUR_SIGMA = 4, 2.0
# the Bresenham circle of radius 3, contiguous
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]


def reflect101(p, n):
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def blur_taps():
    x = np.arange(-BLUR_R, BLUR_R + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * BLUR_SIGMA * BLUR_SIGMA))
    return (g / g.sum()).astype(F32)


def blur(img):
    """GaussianBlur(9 x 9, sigma 2), BORDER_REFLECT_101: row pass then column pass in float32, taps summed in order, every
    product and sum rounded on its own; half-to-even rounding, saturated"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    k = blur_taps()
    src = img.astype(F32)
    xs = [reflect101(np.arange(W) + d, W) for d in range(-BLUR_R, BLUR_R + 1)]
    ys = [reflect101(np.arange(H) + d, H) for d in range(-BLUR_R, BLUR_R + 1)]
    row = k[0] * src[:, xs[0]]
    for i in range(1, 2 * BLUR_R + 1):
        row = (row + k[i] * src[:, xs[i]]).astype(F32)
    col = k[0] * row[ys[0], :]
    for i in range(1, 2 * BLUR_R + 1):
        col = (col + k[i] * row[ys[i], :]).astype(F32)
    assert row.dtype == F32 and col.dtype == F32
    return np.clip(np.rint(col), 0, 255).astype(np.uint8)


def fast_scores(img, threshold):
    """the score plane [H][W] int: max(A, B) - 1 for a corner at `threshold`, 0 elsewhere (and within 3 pixels of a border)"""
    img = np.asarray(img, np.uint8).astype(np.int32)
    H, W = img.shape
    out = np.zeros((H, W), np.int32)
    if H < 7 or W < 7:
        return out
    v = img[3:H - 3, 3:W - 3]
    d = np.stack([v - img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in CIRCLE])     # [16][h][w]
    dd = np.concatenate([d, d[:8]])
    A = np.full(v.shape, -255, np.int32)
    B = np.full(v.shape, -255, np.int32)
    for k in range(16):
        arc = dd[k:k + 9]
        A = np.maximum(A, arc.min(axis=0))
        B = np.maximum(B, (-arc).min(axis=0))
    best = np.maximum(A, B)
    out[3:H - 3, 3:W - 3] = np.where(best > threshold, best - 1, 0)
    return out


def fast(img, threshold=20):
    """cv::FAST(img, keypoints, threshold, true) -> (keypoints [k][2] float32 (x, y) in raster order, scores [k] int, plane)"""
    s = fast_scores(img, threshold)
    H, W = s.shape
    p = np.pad(s, 1)
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s > p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ys, xs = np.nonzero(keep)            # row-major: rows top to bottom, x ascending
    return np.stack([xs, ys], axis=1).astype(F32).reshape(-1, 2), s[ys, xs], s


def lift(cam, pts):
    """keypoints_norm: liftProjective of the pixel, x / z and y / z rounded to float"""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    mx, my = pt_ref.lift_projective(cam, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    return np.stack([mx.astype(F32), my.astype(F32)], axis=1).reshape(-1, 2)


def _coord(p, off, n):
    """(int)(p + off) in float, toward zero -> (index, inside)"""
    s = (np.asarray(p, F32)[:, None] + np.asarray(off, np.int32).astype(F32)[None, :]).astype(F32)
    fin = (s > F32(-2.0 ** 30)) & (s < F32(2.0 ** 30))
    i = np.trunc(np.where(fin, s, 0)).astype(np.int64)
    return i, fin & (i >= 0) & (i < n)


def brief(blurred, pts, pattern):
    """DVision::BRIEF::compute on the blurred plane -> [k][4] uint64; pattern = (x1, y1, x2, y2), 256 integers each"""
    blurred = np.asarray(blurred, np.uint8)
    H, W = blurred.shape
    pts = np.asarray(pts, F32).reshape(-1, 2)
    x1, y1, x2, y2 = (np.asarray(a, np.int32) for a in pattern)
    assert len(x1) == 256
    ax1, ix1 = _coord(pts[:, 0], x1, W)
    ay1, iy1 = _coord(pts[:, 1], y1, H)
    ax2, ix2 = _coord(pts[:, 0], x2, W)
    ay2, iy2 = _coord(pts[:, 1], y2, H)
    inside = ix1 & iy1 & ix2 & iy2
    c = lambda a, n: np.clip(a, 0, n - 1)
    bits = inside & (blurred[c(ay1, H), c(ax1, W)] < blurred[c(ay2, H), c(ax2, W)])
    return pack_bits(bits)


def pack_bits(bits):
    """[k][256] bool -> [k][4] uint64, bit i at bit i % 64 of word i / 64"""
    bits = np.asarray(bits, bool).reshape(-1, 4, 64)
    w = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, None, :])
    return np.bitwise_or.reduce(w, axis=2)


def unpack_bits(desc):
    desc = np.asarray(desc, np.uint64).reshape(-1, 4)
    return (((desc[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)) != 0).reshape(-1, 256)


def match(window_brief, old_brief, old_kp, old_norm):
    """searchByBRIEFDes -> (matched_2d_old [n][2], matched_2d_old_norm [n][2] float32, status [n] uint8, best_dist [n],
    best_index [n] int32)"""
    wb, ob = unpack_bits(window_brief), unpack_bits(old_brief)
    old_kp, old_norm = np.asarray(old_kp, F32).reshape(-1, 2), np.asarray(old_norm, F32).reshape(-1, 2)
    n = len(wb)
    m2d, m2n = np.zeros((n, 2), F32), np.zeros((n, 2), F32)
    status, bd, bi = np.zeros(n, np.uint8), np.full(n, 128, np.int32), np.full(n, -1, np.int32)
    if len(ob):
        dist = (wb[:, None, :] != ob[None, :, :]).sum(axis=2)        # [n][m]
        for i in range(n):
            j = int(np.argmin(dist[i]))                               # the first index of the least distance
            if dist[i, j] < 128:
                bd[i], bi[i] = dist[i, j], j
                if dist[i, j] < 80:
                    status[i], m2d[i], m2n[i] = 1, old_kp[j], old_norm[j]
    return m2d, m2n, status, bd, bi


def reduce_vector(v, status):
    """reduceVector (keyframe.cpp:3-11)"""
    v, status = np.asarray(v), np.asarray(status)
    assert len(v) == len(status)
    return v[status != 0]


# ---- loop verification: KeyFrame::findConnection from the PnP on (keyframe.cpp:406-516) ------------------------------------------
FEW_POINTS, NO_MODEL, NUMERIC, FEW_INLIERS, REJECTED, CLOSED = 0, 1, 2, 3, 4, 5      # VPL_LOOP_*
MIN_LOOP_NUM, MAX_ITERS, REPROJ_ERROR, CONFIDENCE, MAX_YAW_DEG, MAX_T = 25, 100, 10.0 / 460.0, 0.99, 30.0, 20.0
_M64 = (1 << 64) - 1


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(seed, cand, it, counter, n):
    """draw `counter` of iteration `it` of candidate `cand` (csrc/init_relpose_plan.h), in Python integers"""
    h = _mix(seed & _M64)
    for v in (cand, it, counter):
        h = _mix(h ^ (v & 0xFFFFFFFF))
    return ((h >> 32) * n) >> 32


def sample5(seed, it, n):
    idx, counter = [], 0
    while len(idx) < 5:
        d = draw(seed, 0, it, counter, n)
        counter += 1
        if d not in idx:
            idx.append(d)
    return idx


def niters_after(n, good, confidence=CONFIDENCE, max_iters=MAX_ITERS):
    """RANSACUpdateNumIters(confidence, (n - good) / n, 5, max_iters)"""
    import math
    import sys
    p = min(max(confidence, 0.0), 1.0)
    ep = min(max((n - good) / n, 0.0), 1.0)
    num = max(1.0 - p, sys.float_info.min)
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < sys.float_info.min:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def r2ypr_yaw(R):
    """Utility::R2ypr(R).x, degrees"""
    return np.arctan2(R[1, 0], R[0, 0]) / np.pi * 180


def normalize_angle(d):
    return d - 360 * np.floor((d + 180) / 360) if d > 0 else d + 360 * np.floor((-d + 180) / 360)


def verify(pts3d, old_norm, vio_T, vio_R, tic, qic, seed, dt, min_loop_num=MIN_LOOP_NUM, max_iters=MAX_ITERS,
           reproj_error=REPROJ_ERROR, confidence=CONFIDENCE, max_yaw_deg=MAX_YAW_DEG, max_t=MAX_T):
    """the plain sequential RANSAC over the stream, computed in `dt` (np.float64 or np.longdouble) -> dict has_loop, stage,
    ransac_iterations, best_inliers, lm_iterations, lm_termination, status [N], PnP_T_old, PnP_R_old, loop_info"""
    import sfm_ref
    X = np.asarray(pts3d, np.float32).reshape(-1, 3).astype(dt)
    uv = np.asarray(old_norm, np.float32).reshape(-1, 2).astype(dt)
    N = len(X)
    out = dict(has_loop=0, stage=FEW_POINTS, ransac_iterations=0, best_inliers=0, lm_iterations=0, lm_termination=0,
               status=np.zeros(N, np.uint8), PnP_T_old=np.zeros(3, dt), PnP_R_old=np.zeros((3, 3), dt), loop_info=np.zeros(8, dt))
    if not N > min_loop_num:
        return out
    vio_T, tic = np.asarray(vio_T, np.float64).astype(dt), np.asarray(tic, np.float64).astype(dt)
    vio_R, qic = np.asarray(vio_R, np.float64).astype(dt), np.asarray(qic, np.float64).astype(dt)
    Rwc, Twc = vio_R @ qic, vio_T + vio_R @ tic
    q0 = sfm_ref.qnormalized(sfm_ref.mat2q(Rwc.T, dt))
    t0 = -(Rwc.T @ Twc)
    thr2 = dt(np.float64(reproj_error) * np.float64(reproj_error))      # one float64 number for every dtype, as on the device

    def mask_of(q, t):
        R = sfm_ref.qmat(q / np.sqrt(q @ q))
        c = X @ R.T + t
        ex, ey = c[:, 0] / c[:, 2] - uv[:, 0], c[:, 1] / c[:, 2] - uv[:, 1]
        return ex * ex + ey * ey <= thr2

    niters, best_good, best, it = max_iters, 0, None, 0
    while it < niters:
        idx = np.asarray(sample5(seed, it, N))
        r = sfm_ref.pnp(q0, t0, X, idx, uv[idx], dt)
        it += 1
        q, t = r["q"][0], r["t"][0]
        if r["termination"] == sfm_ref.FAILURE or not (np.isfinite(q).all() and np.isfinite(t).all()):
            continue
        m = mask_of(q, t)
        good = int(m.sum())
        if good > max(best_good, 4):
            best_good, best = good, (q, t, m)
            niters = min(niters, niters_after(N, good, confidence, max_iters))
    out.update(ransac_iterations=it, best_inliers=best_good)
    if best is None:
        out["stage"] = NO_MODEL
        return out
    q, t, m = best
    out["status"] = m.astype(np.uint8)
    inl = np.nonzero(m)[0]
    r = sfm_ref.pnp(q, t, X, inl, uv[inl], dt)
    out.update(lm_iterations=r["iterations"], lm_termination=r["termination"])
    q, t = r["q"][0], r["t"][0]
    if r["termination"] == sfm_ref.FAILURE or not (np.isfinite(q).all() and np.isfinite(t).all()):
        out["stage"] = NUMERIC
        return out
    Rpnp = sfm_ref.qmat(q / np.sqrt(q @ q))
    Rwc_old = Rpnp.T
    Rold = Rwc_old @ qic.T
    Told = Rwc_old @ (-t) - Rold @ tic
    out.update(PnP_R_old=Rold, PnP_T_old=Told)
    if not best_good > min_loop_num:
        out["stage"] = FEW_INLIERS
        return out
    rt = Rold.T @ (vio_T - Told)
    rq = sfm_ref.mat2q(Rold.T @ vio_R, dt)
    yaw = normalize_angle(r2ypr_yaw(vio_R) - r2ypr_yaw(Rold))
    out["loop_info"] = np.concatenate([rt, rq, [yaw]]).astype(dt)
    ok = abs(yaw) < max_yaw_deg and np.sqrt(rt @ rt) < max_t
    out.update(has_loop=int(ok), stage=CLOSED if ok else REJECTED)
    return out
