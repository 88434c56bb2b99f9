"""NumPy restatement of the point front-end's stages (the reference of tests/test_pt_reference.py and
tests/test_gpu_pt_stages.py).  Float32 wherever the tracker's OpenCV calls compute in float, in the order written
here; the same order is stated in vplines-slam_amd/csrc/pt_kernels.h, which implements exactly it.

detect(): cvmodified::goodFeaturesToTrack (feature_tracker/src/cvmodified/cvmodified.cpp:38-216) as detect_features calls
it -- blockSize 3, gradientSize 3, no Harris, qualityLevel 0.01.  What OpenCV leaves to its build ("unpinned"):
  * Sobel 3 x 3 on 8-bit input, output float, scale s = float32(1 / (2^(aperture-1) * blockSize * 255)) = float32(1 / 3060)
    folded into the SMOOTHING taps (s, 2s, s), the differencing taps stay (-1, 0, 1); rows first, then columns:
      Dx = 2s * d[y] + s * (d[y-1] + d[y+1])   with d = p[x+1] - p[x-1]              (exact integers in float)
      Dy = r[y+1] - r[y-1]                      with r = 2s * p[x] + s * (p[x-1] + p[x+1])
    every product and sum rounded to float32 on its own (no fused multiply-add), BORDER_REFLECT_101 on the image;
  * the three products Dx Dx, Dx Dy, Dy Dy rounded to float32, their unnormalised 3 x 3 box sums accumulated in double
    (row by row, left to right) and rounded to float32 once, BORDER_REFLECT_101 on the product planes;
  * a = 0.5 Sxx, b = Sxy, c = 0.5 Syy;  eig = (a + c) - sqrt((a - c)^2 + b^2), float32 throughout, the root correctly rounded.
    (Equal bit for bit to 0.5 (Sxx + Syy) - sqrt(0.25 (Sxx - Syy)^2 + Sxy^2): halving is exact.)
"""
import numpy as np

F32 = np.float32
QUALITY_LEVEL = 0.01
SOBEL_SCALE = F32(1.0 / 3060.0)


def _reflect101(a):
    """the plane with one reflected pixel on every side (BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba)"""
    return np.pad(a, 1, mode="reflect")


def min_eig_plane(img):
    """cornerMinEigenVal(img, blockSize 3, ksize 3) of an 8-bit image: float32 [H][W]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2 and img.shape[0] >= 2 and img.shape[1] >= 2
    p = _reflect101(img.astype(F32))
    s, s2 = SOBEL_SCALE, F32(2) * SOBEL_SCALE
    d = p[:, 2:] - p[:, :-2]                                    # [H+2][W]
    dx = s2 * d[1:-1] + s * (d[:-2] + d[2:])
    r = s2 * p[:, 1:-1] + s * (p[:, :-2] + p[:, 2:])            # [H+2][W]
    dy = r[2:] - r[:-2]
    assert dx.dtype == F32 and dy.dtype == F32
    out = []
    for prod in (dx * dx, dx * dy, dy * dy):
        q = _reflect101(prod).astype(np.float64)
        acc = np.zeros(img.shape, np.float64)
        for j in range(3):
            for i in range(3):
                acc = acc + q[j:j + img.shape[0], i:i + img.shape[1]]
        out.append(acc.astype(F32))
    a, b, c = out[0] * F32(0.5), out[1], out[2] * F32(0.5)
    amc = a - c
    eig = (a + c) - np.sqrt(amc * amc + b * b)
    assert eig.dtype == F32
    return eig


def corner_candidates(eig, mask=None):
    """minMaxLoc under the mask, THRESH_TOZERO at 0.01 max, 3 x 3 dilation, the test of cvmodified.cpp:78-93.
    Returns (linear indices of the candidates in scan order, the thresholded plane)."""
    H, W = eig.shape
    if mask is None:
        max_val = float(eig.max())
    else:
        m = np.asarray(mask) != 0
        max_val = float(eig[m].max()) if m.any() else 0.0
    thresh = F32(max_val * QUALITY_LEVEL)                       # threshold() takes a double and compares in float
    t = np.where(eig > thresh, eig, F32(0))
    dil = np.full((H, W), -np.inf, F32)
    q = np.pad(t, 1, mode="constant", constant_values=-np.inf)
    for j in range(3):
        for i in range(3):
            dil = np.maximum(dil, q[j:j + H, i:i + W])
    ok = (t != 0) & (t == dil)
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return np.flatnonzero(ok.ravel()), t


def cv_round(v):
    """cvRound of a double: to nearest, ties to even"""
    return int(np.rint(v))


def detect(img, max_corners, min_distance, mask=None, return_total=False):
    """goodFeaturesToTrack: corners [n][2] float32 (x, y) in the order kept, scores [n] float32"""
    assert max_corners >= 1
    eig = min_eig_plane(img)
    H, W = eig.shape
    idx, t = corner_candidates(eig, mask)
    val = t.ravel()[idx]
    # greaterThanPtr (:16-21): descending by value, equal values by descending address
    order = np.lexsort((-idx, -val.astype(np.float64)))
    idx, val = idx[order], val[order]
    xs, ys = (idx % W).astype(np.int64), (idx // W).astype(np.int64)
    corners, scores = [], []
    if min_distance >= 1:
        cell = cv_round(min_distance)
        gw, gh = (W + cell - 1) // cell, (H + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for x, y, v in zip(xs, ys, val):
            xc, yc = int(x) // cell, int(y) // cell
            good = True
            for yy in range(max(0, yc - 1), min(gh - 1, yc + 1) + 1):
                for xx in range(max(0, xc - 1), min(gw - 1, xc + 1) + 1):
                    for (mx, my) in grid[yy * gw + xx]:
                        if float((x - mx) * (x - mx) + (y - my) * (y - my)) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((int(x), int(y)))
                corners.append((x, y))
                scores.append(v)
                if len(corners) == max_corners:
                    break
    else:
        for x, y, v in list(zip(xs, ys, val))[:max_corners]:
            corners.append((x, y))
            scores.append(v)
    c = np.array(corners, F32).reshape(-1, 2)
    s = np.array(scores, F32)
    return (c, s, len(idx)) if return_total else (c, s)


def circle_half_widths(r):
    """The pixel set of a filled circle of integer radius r as OpenCV's integer midpoint walk fills it (imgproc/drawing.cpp,
    Circle(): err = 0, dx = r, dy = 0, plus = 1, minus = 2 r - 1; each step fills rows cy -+ dy over cx -+ dx and rows
    cy -+ dx over cx -+ dy).  Returns hw [2r+1]: row cy + (j - r) covers cx - hw[j] .. cx + hw[j].
    Restated from the algorithm's description; it is not pinned against a run of cv::circle."""
    hw = np.zeros(2 * r + 1, np.int32)
    err, dx, dy, plus, minus = 0, r, 0, 1, (r << 1) - 1
    while dx >= dy:
        for row, half in ((dy, dx), (dx, dy)):
            hw[r + row] = max(hw[r + row], half)
            hw[r - row] = max(hw[r - row], half)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1   # 0 while the error stays non-positive, else all ones: dx steps inwards
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return hw


def disc_mask(H, W, centres, r, base=None):
    """a mask plane (255 = free) with a filled circle of radius r set to 0 around every centre (setMask's cv::circle)"""
    m = np.full((H, W), 255, np.uint8) if base is None else np.array(base, np.uint8)
    hw = circle_half_widths(r)
    for cx, cy in centres:
        for j in range(2 * r + 1):
            y = cy + j - r
            if 0 <= y < H:
                m[y, max(0, cx - hw[j]):min(W, cx + hw[j] + 1)] = 0
    return m


# ---- the camera model: PinholeCamera with k1, k2, p1, p2 (camera_model/src/camera_models/PinholeCamera.cc) ----------------
import collections

Camera = collections.namedtuple("Camera", "fx fy cx cy k1 k2 p1 p2")
EUROC_CAM0 = Camera(458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def distortion(cam, x, y):
    """PinholeCamera::distortion (:646-662), float64, the products in the source's order"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = cam.k1 * rho2 + cam.k2 * rho2 * rho2
    return (x * rad + 2.0 * cam.p1 * mxy + cam.p2 * (rho2 + 2.0 * mx2),
            y * rad + 2.0 * cam.p2 * mxy + cam.p1 * (rho2 + 2.0 * my2))


def lift_projective(cam, u, v, steps=8):
    """PinholeCamera::liftProjective (:450-510): pixel -> the ray (mx, my, 1) by the recursive distortion removal"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    ik11, ik13, ik22, ik23 = 1.0 / cam.fx, -cam.cx / cam.fx, 1.0 / cam.fy, -cam.cy / cam.fy
    mx_d, my_d = ik11 * u + ik13, ik22 * v + ik23
    dx, dy = distortion(cam, mx_d, my_d)
    mx, my = mx_d - dx, my_d - dy
    for _ in range(1, steps):
        dx, dy = distortion(cam, mx, my)
        mx, my = mx_d - dx, my_d - dy
    return mx, my


def space_to_plane(cam, x, y):
    """PinholeCamera::spaceToPlane (:519-542) of the ray (x, y, 1): the distorted pixel"""
    dx, dy = distortion(cam, x, y)
    return cam.fx * (np.asarray(x, np.float64) + dx) + cam.cx, cam.fy * (np.asarray(y, np.float64) + dy) + cam.cy


def virtual_pinhole(cam, pts, W, H, focal=460.0):
    """rejectWithF's re-projection (feature_tracker.cpp:233-245): [n][2] float32 pixels -> [n][2] cv::Point2f"""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    mx, my = lift_projective(cam, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    return np.stack([(focal * mx + W / 2.0).astype(F32), (focal * my + H / 2.0).astype(F32)], axis=1)


def reject_f(cur, forw, cam, W, H, samples, focal=460.0, f_threshold=1.0):
    """rejectWithF (:226-261) -> status [n] uint8.  samples(N): the [1000][7] sample table of a list of N points (the device's
    stream: vpl_relpose_debug_plan with candidate 0).  The RANSAC is tests/relpose_ref.py's, run with this threshold."""
    import relpose_ref
    cur, forw = np.asarray(cur, F32).reshape(-1, 2), np.asarray(forw, F32).reshape(-1, 2)
    N = len(cur)
    assert len(forw) == N
    if N < 8:
        return np.ones(N, np.uint8)
    pts = np.concatenate([virtual_pinhole(cam, cur, W, H, focal), virtual_pinhole(cam, forw, W, H, focal)], axis=1).astype(np.float64)
    saved = relpose_ref.THRESHOLD2
    relpose_ref.THRESHOLD2 = float(f_threshold) * float(f_threshold)     # inlier_mask reads the module's threshold
    try:
        r = relpose_ref.ransac(pts, np.asarray(samples(N)), relpose_ref.niters_table(N))
    finally:
        relpose_ref.THRESHOLD2 = saved
    return r["mask"].astype(np.uint8)


# ---- calcOpticalFlowPyrLK(21 x 21, maxLevel 3) ---------------------------------------------------------------------------
LK_WIN, LK_LEVELS, LK_MAXCOUNT = 21, 4, 30
LK_EPS2 = min(max(0.01, 0.0), 10.0) ** 2          # criteria.epsilon, squared as calcOpticalFlowPyrLK does
LK_MIN_EIG = F32(1e-4)
FLT_EPSILON = F32(1.1920928955078125e-07)
FLT_SCALE = F32(1.0 / (1 << 20))


def pyr_down(img):
    """cv::pyrDown of an 8-bit image: [1 4 6 4 1]^2 / 256 rounded, BORDER_REFLECT_101, ((w + 1) / 2, (h + 1) / 2)"""
    H, W = img.shape
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    k = (1, 4, 6, 4, 1)
    oh, ow = (H + 1) // 2, (W + 1) // 2
    acc = np.zeros((oh, ow), np.int64)
    for j in range(5):
        for i in range(5):
            acc += k[j] * k[i] * p[j:j + 2 * oh:2, i:i + 2 * ow:2]
    return ((acc + 128) >> 8).astype(np.uint8)


def scharr(img):
    """calcSharrDeriv: (dx, dy) int16 planes, 3 / 10 / 3 smoothing across, BORDER_REFLECT_101"""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    sm = 3 * (p[:-2, :] + p[2:, :]) + 10 * p[1:-1, :]           # vertical smoothing, [H][W+2]
    dx = sm[:, 2:] - sm[:, :-2]
    d = p[2:, :] - p[:-2, :]                                     # vertical difference, [H][W+2]
    dy = 3 * (d[:, :-2] + d[:, 2:]) + 10 * d[:, 1:-1]
    return dx.astype(np.int16), dy.astype(np.int16)


def lk_pyramid(img, win=LK_WIN, levels=LK_LEVELS):
    """buildOpticalFlowPyramid: levels halved until `levels` stand or the next would be no larger than the window.  Per level
    (pixels padded by `win` with BORDER_REFLECT_101, dx and dy padded with zeros), all int64"""
    out = []
    cur = np.asarray(img, np.uint8)
    for l in range(levels):
        dx, dy = scharr(cur)
        out.append((np.pad(cur.astype(np.int64), win, mode="reflect"), np.pad(dx.astype(np.int64), win), np.pad(dy.astype(np.int64), win),
                    cur.shape[1], cur.shape[0]))
        nw, nh = (cur.shape[1] + 1) // 2, (cur.shape[0] + 1) // 2
        if nw <= win or nh <= win:
            break
        cur = pyr_down(cur)
    return out


def _lk_weights(a, b):
    """iw00 .. iw11 from the float remainders (cvRound: to nearest even)"""
    one = F32(1)
    w00 = int(np.rint((one - a) * (one - b) * F32(1 << 14)))
    w01 = int(np.rint(a * (one - b) * F32(1 << 14)))
    w10 = int(np.rint((one - a) * b * F32(1 << 14)))
    return w00, w01, w10, (1 << 14) - w00 - w01 - w10


def _rows_then_column(t):
    """the stated summation order: each window row left to right, then the row sums top to bottom, all in float32"""
    rows = np.cumsum(t.astype(F32), axis=1, dtype=F32)[:, -1]
    return np.cumsum(rows, dtype=F32)[-1]


def _bilinear(plane, x0, y0, w, shift, win):
    a = plane[y0:y0 + win + 1, x0:x0 + win + 1]
    v = a[:-1, :-1] * w[0] + a[:-1, 1:] * w[1] + a[1:, :-1] * w[2] + a[1:, 1:] * w[3]
    return (v + (1 << (shift - 1))) >> shift


def lk_flow(prev_img, next_img, pts, win=LK_WIN):
    """-> (next_pts [n][2] float32, status [n] uint8): lk_tracker_invoker_ori.cpp level by level, err left out"""
    pts = np.asarray(pts, F32).reshape(-1, 2)
    pI, pJ = lk_pyramid(prev_img, win), lk_pyramid(next_img, win)
    n = len(pts)
    nxt = np.zeros((n, 2), F32)
    status = np.ones(n, np.uint8)
    half = F32((win - 1) * 0.5)
    max_level = len(pI) - 1
    for level in range(max_level, -1, -1):
        I, dIx, dIy, w, h = pI[level]
        J = pJ[level][0]
        lscale = F32(1.0 / (1 << level))
        for k in range(n):
            prev = pts[k] * lscale
            nx, ny = (prev[0], prev[1]) if level == max_level else (nxt[k, 0] * F32(2), nxt[k, 1] * F32(2))
            nxt[k] = (nx, ny)
            px, py = prev[0] - half, prev[1] - half
            ipx, ipy = int(np.floor(px)), int(np.floor(py))
            if ipx < -win or ipx >= w or ipy < -win or ipy >= h:
                if level == 0:
                    status[k] = 0
                continue
            wt = _lk_weights(px - F32(ipx), py - F32(ipy))
            Iw = _bilinear(I, ipx + win, ipy + win, wt, 9, win)
            Ix = _bilinear(dIx, ipx + win, ipy + win, wt, 14, win)
            Iy = _bilinear(dIy, ipx + win, ipy + win, wt, 14, win)
            A11 = _rows_then_column(Ix * Ix) * FLT_SCALE
            A12 = _rows_then_column(Ix * Iy) * FLT_SCALE
            A22 = _rows_then_column(Iy * Iy) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4) * A12 * A12)) / F32(2 * win * win)
            if min_eig < LK_MIN_EIG or D < FLT_EPSILON:
                if level == 0:
                    status[k] = 0
                continue
            D = F32(1) / D
            nx, ny = nx - half, ny - half
            pdx = pdy = F32(0)
            j = 0
            while j < LK_MAXCOUNT:
                inx, iny = int(np.floor(nx)), int(np.floor(ny))
                if inx < -half or inx >= w or iny < -half or iny >= h:
                    if level == 0:
                        status[k] = 0
                    break
                wt = _lk_weights(nx - F32(inx), ny - F32(iny))
                diff = _bilinear(J, inx + win, iny + win, wt, 9, win) - Iw
                b1 = _rows_then_column(diff * Ix) * FLT_SCALE
                b2 = _rows_then_column(diff * Iy) * FLT_SCALE
                dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                nx, ny = nx + dx, ny + dy
                nxt[k] = (nx + half, ny + half)
                if float(dx) * float(dx) + float(dy) * float(dy) <= LK_EPS2:
                    break
                if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                    nxt[k] = (nxt[k, 0] - dx * F32(0.5), nxt[k, 1] - dy * F32(0.5))
                    break
                pdx, pdy = dx, dy
                j += 1
            if j == LK_MAXCOUNT and level == 0:
                status[k] = 0
            if status[k] and level == 0:           # the range test in front of the err loop
                fx, fy = nxt[k, 0] - half, nxt[k, 1] - half
                ix, iy = int(np.floor(fx)), int(np.floor(fy))
                if ix < -win or ix >= w or iy < -win or iy >= h:
                    status[k] = 0
    return nxt, status


# ---- FeatureTracker::readImage + updateID ---------------------------------------------------------------------------------
class PointTracker:
    """one camera of the reference's tracker on frames that are already equalised.  setMask orders stably (the earlier list
    position first among equal track_cnt); samples(seed, N) is the RANSAC's sample table."""

    def __init__(self, cam, W, H, samples, max_cnt=150, min_dist=30, f_threshold=1.0, focal=460.0, next_id=0):
        self.cam, self.W, self.H, self.samples = cam, W, H, samples
        self.max_cnt, self.min_dist, self.f_threshold, self.focal = max_cnt, min_dist, f_threshold, focal
        self.n_id = next_id
        self.base_mask = None      # the fisheye mask setMask starts from
        self.reset()

    def reset(self):
        self.cur_img = None
        self.pts, self.ids, self.cnt, self.sc = np.zeros((0, 2), F32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F32)
        self.prev_map, self.prev_time = {}, 0.0

    def read_image(self, img, t, publish, seed):
        """-> dict res (the six counts), ids, rows [k][7]"""
        res = dict(tracked=0, after_border=0, after_f=0, after_mask=0, detected=0, published=0)
        cur, pts, ids, cnt, sc = self.pts, self.pts, self.ids, self.cnt, self.sc
        if len(self.pts):
            forw, st = lk_flow(self.cur_img, img, self.pts)
            res["tracked"] = int(st.sum())
            x, y = np.rint(forw[:, 0]).astype(np.int64), np.rint(forw[:, 1]).astype(np.int64)
            ok = (st != 0) & (1 <= x) & (x < self.W - 1) & (1 <= y) & (y < self.H - 1)
            cur, pts, ids, cnt, sc = self.pts[ok], forw[ok], ids[ok], cnt[ok], sc[ok]
        cnt = cnt + 1
        res["after_border"] = len(pts)
        if publish:
            keep = reject_f(cur, pts, self.cam, self.W, self.H, lambda N: self.samples(seed, N), self.focal, self.f_threshold) != 0
            pts, ids, cnt, sc = pts[keep], ids[keep], cnt[keep], sc[keep]
        res["after_f"] = len(pts)
        if publish:
            order = np.argsort(-cnt, kind="stable")
            mask = np.full((self.H, self.W), 255, np.uint8) if self.base_mask is None else np.array(self.base_mask, np.uint8)
            hw = circle_half_widths(self.min_dist)
            kept = []
            for k in order:
                cx, cy = int(np.rint(pts[k, 0])), int(np.rint(pts[k, 1]))
                if mask[cy, cx] == 255:
                    kept.append(k)
                    for j in range(2 * self.min_dist + 1):
                        yy = cy + j - self.min_dist
                        if 0 <= yy < self.H:
                            mask[yy, max(0, cx - hw[j]):min(self.W, cx + hw[j] + 1)] = 0
            kept = np.array(kept, np.int64)
            pts, ids, cnt, sc = pts[kept], ids[kept], cnt[kept], sc[kept]
            res["after_mask"] = len(pts)
            want = self.max_cnt - len(pts)
            if want > 0:
                c, s = detect(img, want, float(self.min_dist), mask)
                res["detected"] = len(c)
                pts, ids = np.concatenate([pts, c]), np.concatenate([ids, -np.ones(len(c), np.int64)])
                cnt, sc = np.concatenate([cnt, np.ones(len(c), np.int64)]), np.concatenate([sc, s])
        else:
            res["after_mask"] = len(pts)
        pts, sc = pts.astype(F32).reshape(-1, 2), sc.astype(F32)
        # undistortedPoints
        mx, my = lift_projective(self.cam, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
        un = np.stack([mx.astype(F32), my.astype(F32)], axis=1).reshape(-1, 2)
        max_prob = sc.max() if len(sc) else F32(1)
        usc = sc / max_prob
        vel = np.zeros((len(pts), 2), F32)
        dt = t - self.prev_time
        if self.prev_map:
            for i in range(len(pts)):
                if ids[i] != -1 and int(ids[i]) in self.prev_map:
                    p = self.prev_map[int(ids[i])]
                    vel[i] = (F32(float(un[i, 0] - p[0]) / dt), F32(float(un[i, 1] - p[1]) / dt))
        new_map = {}
        for i in range(len(pts)):
            new_map.setdefault(int(ids[i]), un[i].copy())
        self.prev_map, self.prev_time = new_map, t
        # updateID
        ids = ids.copy()
        for i in range(len(ids)):
            if ids[i] == -1:
                ids[i] = self.n_id
                self.n_id += 1
        self.cur_img, self.pts, self.ids, self.cnt, self.sc, self.un, self.usc = img, pts, ids, cnt, sc, un, usc
        rows = np.zeros((0, 7))
        rid = np.zeros(0, np.int64)
        if publish:
            sel = cnt > 1
            prob = float(usc[0]) if len(usc) else 0.0
            rows = np.concatenate([un[sel].astype(np.float64), pts[sel].astype(np.float64), vel[sel].astype(np.float64),
                                   np.full((int(sel.sum()), 1), prob)], axis=1)
            rid = ids[sel]
            res["published"] = int(sel.sum())
        return dict(res=res, ids=rid, rows=rows)
