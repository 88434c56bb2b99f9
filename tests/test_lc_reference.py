"""tests/lc_ref.py against brute-force restatements written differently (plain loops, one pixel / one bit at a time) on a small
random image, and the host glue of the loop-closure calls.  No GPU."""
import numpy as np
import pytest

import lc_inputs
import lc_ref


def random_image(seed=3, w=32, h=32):
    rng = np.random.RandomState(seed)
    # smooth blobs plus noise: a few dozen FAST corners of mixed polarity
    img = rng.randint(60, 200, (h // 4 + 1, w // 4 + 1)).repeat(4, axis=0).repeat(4, axis=1)[:h, :w] + rng.randint(-12, 13, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def passes(img, x, y, t):
    """FAST 9-16 from its definition: nine contiguous circle pixels all brighter than v + t or all darker than v - t"""
    v = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in lc_ref.CIRCLE]
    for start in range(16):
        arc = [ring[(start + j) % 16] for j in range(9)]
        if all(p > v + t for p in arc) or all(p < v - t for p in arc):
            return True
    return False


def test_fast_score_is_the_largest_passing_threshold():
    img = random_image()
    H, W = img.shape
    t0 = 20
    plane = lc_ref.fast_scores(img, t0)
    n_corners = 0
    for y in range(H):
        for x in range(W):
            if x < 3 or y < 3 or x >= W - 3 or y >= H - 3:
                assert plane[y, x] == 0
                continue
            largest = -1
            for t in range(256):
                if passes(img, x, y, t):
                    largest = t
            # (passing is monotone in t: the search above finds the largest)
            want = largest if largest >= t0 else 0
            assert plane[y, x] == want, (x, y, plane[y, x], largest)
            n_corners += want > 0
    assert n_corners > 10


def test_fast_list_is_the_strict_local_maxima_in_raster_order():
    img = random_image(5)
    kp, sc, plane = lc_ref.fast(img, 20)
    H, W = plane.shape
    want = []
    for y in range(H):
        for x in range(W):
            s = plane[y, x]
            if s > 0 and all(s > plane[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                want.append((x, y))
    assert len(want) > 3 and [tuple(p) for p in kp.astype(int).tolist()] == want
    assert sc.tolist() == [plane[y, x] for x, y in want]


def test_blur_matches_a_per_pixel_restatement():
    img = random_image(9, 19, 11)
    H, W = img.shape
    k = lc_ref.blur_taps()
    assert k.dtype == np.float32 and abs(float(k.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(k, k[::-1])

    def refl(p, n):
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p

    row = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            a = np.float32(k[0]) * np.float32(img[y, refl(x - 4, W)])
            for i in range(1, 9):
                a = np.float32(a + np.float32(k[i] * np.float32(img[y, refl(x - 4 + i, W)])))
            row[y, x] = a
    want = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            a = np.float32(k[0] * row[refl(y - 4, H), x])
            for i in range(1, 9):
                a = np.float32(a + np.float32(k[i] * row[refl(y - 4 + i, H), x]))
            want[y, x] = min(max(int(np.rint(a)), 0), 255)
    assert np.array_equal(lc_ref.blur(img), want)
    assert np.array_equal(lc_ref.blur(np.full((9, 12), 200, np.uint8)), np.full((9, 12), 200, np.uint8))


def test_brief_matches_a_per_bit_restatement():
    img = random_image(4)
    H, W = img.shape
    x1, y1, x2, y2 = lc_inputs.pattern()
    pts = np.array([(16, 16), (0.25, 0.75), (31.5, 30.25), (12.5, 23.75), (23.5, 8.0), (-30.0, 5.0), (20.5, 0.5)], np.float32)
    got = lc_ref.unpack_bits(lc_ref.brief(img, pts, (x1, y1, x2, y2)))
    hit_zero_from_negative = False
    for k, (px, py) in enumerate(pts):
        for i in range(256):
            c = [np.float32(px) + np.float32(x1[i]), np.float32(py) + np.float32(y1[i]), np.float32(px) + np.float32(x2[i]),
                 np.float32(py) + np.float32(y2[i])]
            hit_zero_from_negative |= any(-1 < v < 0 for v in c)
            a, b, cc, d = (int(v) for v in c)      # int(): toward zero, as the C conversion
            inside = 0 <= a < W and 0 <= b < H and 0 <= cc < W and 0 <= d < H
            assert got[k, i] == (inside and img[b, a] < img[d, cc]), (k, i)
    assert hit_zero_from_negative and not got[5].any() and got[0].any()
    # bit i is bit i % 64 of word i / 64
    one = np.zeros((1, 256), bool)
    one[0, 70] = True
    assert lc_ref.pack_bits(one).tolist() == [[0, 1 << 6, 0, 0]]


def test_match_matches_a_sequential_restatement():
    for win, old, okp, onr in lc_inputs.synthetic_match_pairs(tile=64)[:10]:
        m2d, m2n, status, bd, bi = lc_ref.match(win, old, okp, onr)
        for i in range(len(win)):
            best_dist, best_index = 128, -1
            for j in range(len(old)):
                dis = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(win[i], old[j]))
                if dis < best_dist:
                    best_dist, best_index = dis, j
            ok = best_index != -1 and best_dist < 80
            assert (bd[i], bi[i], status[i]) == (best_dist, best_index, int(ok))
            assert m2d[i].tolist() == (okp[best_index].tolist() if ok else [0, 0])
            assert m2n[i].tolist() == (onr[best_index].tolist() if ok else [0, 0])


def test_reduce_vector_and_the_glue_of_loop_matches():
    import vplines_slam_amd as v
    rv = v.frontend.reduce_vector
    a = np.arange(12.0).reshape(6, 2)
    st = np.array([1, 0, 2, 0, 0, 1], np.uint8)
    # reduceVector as written: v[j++] = v[i] for every non-zero status
    want, j = a.copy(), 0
    for i in range(len(a)):
        if st[i]:
            want[j] = a[i]
            j += 1
    assert np.array_equal(rv(a, st), want[:j]) and np.array_equal(lc_ref.reduce_vector(a, st), want[:j])
    assert len(rv(a, np.zeros(6))) == 0
    with pytest.raises(ValueError):
        rv(a, st[:5])

    class FakeFrontend:          # the glue alone: what it hands to lc_match and how it reduces the lists by the status
        def lc_match(self, wb, ob, okp, onr):
            assert len(wb) == len(ob) == len(okp) == len(onr) == 1
            r = lc_ref.match(wb[0], ob[0], okp[0], onr[0])
            return [dict(matched_2d_old=r[0], matched_2d_old_norm=r[1], status=r[2], best_dist=r[3], best_index=r[4])]

    win, old, okp, onr = lc_inputs.glue_pair()
    k = len(win)
    cur = dict(window_brief=win, point_2d_uv=np.arange(2.0 * k).reshape(k, 2), point_2d_norm=np.arange(2.0 * k).reshape(k, 2) / 460,
               point_3d=np.arange(3.0 * k).reshape(k, 3), point_id=np.arange(k) + 100.0)
    r = v.frontend.loop_matches(FakeFrontend(), cur, dict(brief=old, keypoints=okp, keypoints_norm=onr))
    st = r["status"]
    assert st.tolist() == [1, 0, 0, 1, 0, 1]
    for name, src in (("matched_2d_cur", "point_2d_uv"), ("matched_2d_cur_norm", "point_2d_norm"), ("matched_3d", "point_3d"),
                      ("matched_id", "point_id")):
        assert np.array_equal(r[name], lc_ref.reduce_vector(cur[src], st))
    assert np.array_equal(r["matched_2d_old"], okp[[0, 2, 3]])
    with pytest.raises(ValueError):
        v.frontend.loop_matches(FakeFrontend(), dict(cur, point_id=np.arange(k - 1)), dict(brief=old, keypoints=okp, keypoints_norm=onr))


def test_find_connection_chains_match_reduce_and_verify():
    """the host glue alone, with stand-ins for the two contexts: the lists the verification is handed are the ones reduced by the
    match status, and its inliers reduce them again -- unless too few matches were left for it to run"""
    import vplines_slam_amd as v

    class FakeFrontend:
        def lc_match(self, wb, ob, okp, onr):
            r = lc_ref.match(wb[0], ob[0], okp[0], onr[0])
            return [dict(matched_2d_old=r[0], matched_2d_old_norm=r[1], status=r[2], best_dist=r[3], best_index=r[4])]

    class FakeContext:
        def __init__(self, stage, pnp_status):
            self.stage, self.pnp_status, self.seen = stage, np.asarray(pnp_status, np.uint8), None

        def loop_verify(self, inputs, options=None):
            self.seen = inputs[0]
            res = v.LoopResult()
            res.stage, res.has_loop = self.stage, int(self.stage == v.capi.LOOP_CLOSED)
            return [res], [self.pnp_status[:len(inputs[0].pts3d)]]

    win, old, okp, onr = lc_inputs.glue_pair()
    k = len(win)
    cur = dict(window_brief=win, point_2d_uv=np.arange(2.0 * k).reshape(k, 2), point_2d_norm=np.arange(2.0 * k).reshape(k, 2) / 460,
               point_3d=np.arange(3.0 * k).reshape(k, 3), point_id=np.arange(k) + 100.0, origin_vio_T=np.array([1.0, 2.0, 3.0]),
               origin_vio_R=np.eye(3), tic=np.zeros(3), qic=np.eye(3))
    oldkf = dict(brief=old, keypoints=okp, keypoints_norm=onr)
    ctx = FakeContext(v.capi.LOOP_CLOSED, [1, 0, 1])
    r = v.frontend.find_connection(FakeFrontend(), ctx, cur, oldkf, seed=9)
    # what the verification saw: the lists after the match (windows 0, 3, 5), as float
    assert np.array_equal(ctx.seen.pts3d, cur["point_3d"][[0, 3, 5]].astype(np.float32))
    assert np.array_equal(ctx.seen.old_norm, onr[[0, 2, 3]]) and ctx.seen.seed == 9 and np.array_equal(ctx.seen.origin_vio_T, [1, 2, 3])
    assert r["has_loop"] and r["match_status"].tolist() == [1, 0, 0, 1, 0, 1] and r["pnp_status"].tolist() == [1, 0, 1]
    assert r["matched_id"].tolist() == [100.0, 105.0] and np.array_equal(r["matched_2d_old"], okp[[0, 3]])
    assert np.array_equal(r["matched_3d"], cur["point_3d"][[0, 5]])
    # too few matches: nothing ran, the lists stay as the match left them
    ctx = FakeContext(v.capi.LOOP_FEW_POINTS, [0, 0, 0])
    r = v.frontend.find_connection(FakeFrontend(), ctx, cur, oldkf)
    assert not r["has_loop"] and r["pnp_status"] is None and r["matched_id"].tolist() == [100.0, 103.0, 105.0]
