"""The loop-closure front-end's stage calls on the device against tests/lc_ref.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import vplines_slam_amd as v

import lc_inputs
import lc_ref

pytestmark = pytest.mark.gpu

VPL_E_INVALID, VPL_E_CAPACITY = -1, -4
CAM = lc_inputs.CAM


def make_ctx(images, max_keypoints=1024, max_window_points=256, pattern=True):
    n, H, W = images.shape
    fe = v.frontend.FrontendContext(max_images=n, width=W, height=H, max_lines=64)
    fe.lc_reserve(max_keypoints, max_window_points)
    if pattern:
        fe.lc_set_pattern(*lc_inputs.pattern())
    return fe


def camera():
    return v.frontend.PointCamera(*CAM)


@pytest.mark.parametrize("name", ["crop160x120", "crop75x53", "7x7", "constant", "batch3_constant_in_the_middle"])
def test_lc_keyframe_blur_and_fast_match_the_reference_bit_for_bit(name):
    images = lc_inputs.image_cases()[name]
    ref = lc_inputs.ref_keyframe(name)
    fe = make_ctx(images)
    try:
        got = fe.lc_keyframe(images, [np.zeros((0, 2))] * len(images), camera(), lc_inputs.FAST_TH)
        again = fe.lc_keyframe(None, [np.zeros((0, 2))] * len(images), camera(), lc_inputs.FAST_TH)   # the frames in the slots
        for i, (g, (rb, rkp, rsc, rplane, rnorm, rbrief)) in enumerate(zip(got, ref)):
            blurred, score = fe.lc_debug_frame(i)
            print(name, i, "keypoints", len(g["keypoints"]), "ref", len(rkp))
            assert np.array_equal(blurred, rb), "blurred plane of image %d differs" % i
            assert np.array_equal(score.astype(np.int32), rplane), "FAST score plane of image %d differs" % i
            assert g["keypoints"].shape == rkp.shape and np.array_equal(g["keypoints"], rkp), "positions or order differ"
            kx, ky = rkp[:, 0].astype(int), rkp[:, 1].astype(int)
            assert np.array_equal(score[ky, kx].astype(np.int32), rsc)
            assert np.array_equal(g["keypoints_norm"].view(np.uint32), rnorm.view(np.uint32))
            assert np.array_equal(g["brief"], rbrief)
            for k in g:
                assert np.array_equal(g[k], again[i][k]), k
    finally:
        fe.close()
    if name == "7x7":
        assert ref[0][1].tolist() == [[3.0, 3.0]]
    if name == "constant":
        assert len(ref[0][1]) == 0
    if name == "batch3_constant_in_the_middle":
        assert len(ref[1][1]) == 0 and len(ref[0][1]) > 0 and len(ref[2][1]) > 0
    if name in ("crop160x120", "crop75x53"):
        assert len(ref[0][1]) > 64


def test_lc_fast_ties_and_borders():
    img = lc_inputs.ties_and_borders()
    kp, sc, plane = lc_ref.fast(img, lc_inputs.FAST_TH)
    have = {(int(x), int(y)) for x, y in kp}
    # what the input is built for, checked on the reference first
    (ax, ay), (bx, by) = lc_inputs.TIE
    assert plane[ay, ax] == plane[by, bx] > 0 and abs(ax - bx) + abs(ay - by) == 1
    assert lc_inputs.TIE[0] not in have and lc_inputs.TIE[1] not in have
    assert all(c in have for c in lc_inputs.BORDER_CORNERS)
    fe = make_ctx(np.ascontiguousarray(img)[None])
    try:
        g, = fe.lc_keyframe(np.ascontiguousarray(img)[None], [np.zeros((0, 2))], camera(), lc_inputs.FAST_TH)
        _, score = fe.lc_debug_frame(0)
    finally:
        fe.close()
    assert np.array_equal(score.astype(np.int32), plane)
    assert np.array_equal(g["keypoints"], kp)


def test_lc_brief_fractional_window_points_at_the_borders():
    img = lc_inputs.image_cases()["crop160x120"]
    H, W = img.shape[1:]
    pts = lc_inputs.brief_border_points(W, H)
    blurred = lc_inputs.ref_keyframe("crop160x120")[0][0]
    want = lc_ref.brief(blurred, pts, lc_inputs.pattern())
    # the inputs do what they are for: some tests land on column / row 0 from a sum in (-1, 0); the outside points give 0 bits
    x1, y1, x2, y2 = lc_inputs.pattern()
    sums = np.concatenate([(pts[:, 0:1] + x1[None].astype(np.float32)).ravel(), (pts[:, 1:2] + y1[None].astype(np.float32)).ravel()])
    assert ((sums > -1) & (sums < 0)).any()
    assert not want[-3:].any() and want[:-3].any(axis=1).all()
    fe = make_ctx(img)
    try:
        g, = fe.lc_keyframe(img, [pts], camera(), lc_inputs.FAST_TH)
    finally:
        fe.close()
    assert g["window_brief"].shape == want.shape
    bad = np.nonzero((g["window_brief"] != want).any(axis=1))[0]
    assert len(bad) == 0, "window points %s differ" % pts[bad].tolist()


def test_lc_brief_is_the_same_for_both_lists():
    img = lc_inputs.image_cases()["crop75x53"]
    rkp = lc_inputs.ref_keyframe("crop75x53")[0][1]
    fe = make_ctx(img)
    try:
        g, = fe.lc_keyframe(img, [rkp], camera(), lc_inputs.FAST_TH)
    finally:
        fe.close()
    assert len(g["brief"]) == len(rkp) > 0
    assert np.array_equal(g["brief"], g["window_brief"])


def test_lc_keyframe_needs_the_pattern():
    img = lc_inputs.image_cases()["constant"]
    fe = make_ctx(img, pattern=False)
    try:
        with pytest.raises(RuntimeError, match="vpl_lc_set_pattern"):
            fe.lc_keyframe(img, [np.zeros((0, 2))], camera())
        ip = C.POINTER(C.c_int)
        p = [a.ctypes.data_as(ip) for a in lc_inputs.pattern()]
        assert fe.lib.vpl_lc_set_pattern(fe.h, 128, *p) == VPL_E_INVALID
    finally:
        fe.close()


def test_lc_keyframe_refuses_a_keypoint_list_that_overflows():
    images = lc_inputs.image_cases()["crop160x120"]
    ref = lc_inputs.ref_keyframe("crop160x120")[0]
    total = len(ref[1])
    fe = make_ctx(images, max_keypoints=total - 1)
    try:
        KP, WP = total - 1, fe.lc_max_window_points
        out = (np.full((1, KP, 2), -7, np.float32), np.full((1, KP, 2), -7, np.float32), np.full(1, -7, np.int32),
               np.full((1, KP, 4), 7, np.uint64), np.full((1, WP, 4), 7, np.uint64))
        with pytest.raises(RuntimeError) as e:
            fe.lc_keyframe(images, [np.array([[50.0, 50.0]])], camera(), lc_inputs.FAST_TH, out=out)
        assert "(%d)" % VPL_E_CAPACITY in str(e.value) and str(total) in str(e.value)
        assert all((a == -7).all() for a in out[:3]) and all((a == 7).all() for a in out[3:])   # nothing truncated, nothing written
    finally:
        fe.close()
    # one more entry and the same frame passes
    fe = make_ctx(images, max_keypoints=total)
    try:
        g, = fe.lc_keyframe(images, [np.zeros((0, 2))], camera(), lc_inputs.FAST_TH)
        assert np.array_equal(g["keypoints"], ref[1]) and np.array_equal(g["brief"], ref[5])
    finally:
        fe.close()


def check_match(got, want):
    m2d, m2n, status, bd, bi = want
    assert np.array_equal(got["status"], status)
    assert np.array_equal(got["best_dist"], bd) and np.array_equal(got["best_index"], bi)
    assert np.array_equal(got["matched_2d_old"].view(np.uint32), m2d.view(np.uint32))
    assert np.array_equal(got["matched_2d_old_norm"].view(np.uint32), m2n.view(np.uint32))


def test_lc_match_real_descriptors_of_two_displaced_crops():
    a, b = lc_inputs.displaced_pair()
    imgs = np.stack([a, b])
    fe = make_ctx(imgs, max_keypoints=2048)
    try:
        ka, kb = fe.lc_keyframe(imgs, [np.zeros((0, 2))] * 2, camera(), lc_inputs.FAST_TH)
        win = ka["keypoints"][::5][:150]                       # a window's worth of the first crop's corners
        wa, _ = fe.lc_keyframe(None, [win, np.zeros((0, 2))], camera(), lc_inputs.FAST_TH)
        got, = fe.lc_match([wa["window_brief"]], [kb["brief"]], [kb["keypoints"]], [kb["keypoints_norm"]])
    finally:
        fe.close()
    want = lc_ref.match(wa["window_brief"], kb["brief"], kb["keypoints"], kb["keypoints_norm"])
    check_match(got, want)
    # the content moved by (5, -3): most accepted matches say so
    ok = got["status"] == 1
    moved = got["matched_2d_old"][ok] - win[ok]
    print("accepted", int(ok.sum()), "of", len(win), "displaced by (5, -3):", int((moved == (5, -3)).all(axis=1).sum()))
    assert ok.sum() > len(win) // 2 and (moved == (5, -3)).all(axis=1).sum() > 0.8 * ok.sum()


def test_lc_match_synthetic_descriptors():
    pairs = lc_inputs.synthetic_match_pairs(tile=1024)
    want = [lc_ref.match(*p) for p in pairs]
    # the cases are what they claim to be
    assert [int(w[3][0]) for w in want[:7]] == [79, 80, 127, 128, 40, 33, 0]
    assert [int(w[2][0]) for w in want[:7]] == [1, 0, 0, 0, 1, 1, 1] and [int(w[4][0]) for w in want[:7]] == [1, 0, 0, -1, 1, 1, 1]
    assert want[7][4][:3].tolist() == [1024 + 17, 5, 1024] and want[7][3][:3].tolist() == [12, 30, 59] and len(pairs[7][1]) > 1024
    assert (want[8][4] == -1).all() and len(want[9][2]) == 0
    fe = v.frontend.FrontendContext(max_images=len(pairs), width=64, height=48, max_lines=64)
    fe.lc_reserve(1500, 160)
    try:
        for order in (list(range(len(pairs))), [10, 7, 3, 9, 0, 8, 5, 1, 6, 2, 4]):
            got = fe.lc_match(*[[pairs[i][k] for i in order] for k in range(4)])
            for g, i in zip(got, order):
                check_match(g, want[i])
        with pytest.raises(RuntimeError) as e:       # a list longer than the reserved row is refused, not cut
            fe.lc_match([pairs[0][0]], [np.zeros((1501, 4), np.uint64)], [np.zeros((1501, 2))], [np.zeros((1501, 2))])
        assert "(%d)" % VPL_E_CAPACITY in str(e.value)
    finally:
        fe.close()


def test_loop_matches_chains_match_and_reduce_vector():
    win, old, okp, onr = lc_inputs.glue_pair()
    k = len(win)
    cur = dict(window_brief=win, point_2d_uv=np.arange(2 * k, dtype=np.float32).reshape(k, 2),
               point_2d_norm=np.arange(2 * k, dtype=np.float32).reshape(k, 2) / 460, point_3d=np.arange(3.0 * k).reshape(k, 3),
               point_id=np.arange(k) + 100.0)
    fe = v.frontend.FrontendContext(max_images=1, width=64, height=48, max_lines=64)
    fe.lc_reserve(64, 16)
    try:
        r = v.frontend.loop_matches(fe, cur, dict(brief=old, keypoints=okp, keypoints_norm=onr))
    finally:
        fe.close()
    keep = [0, 3, 5]
    assert r["status"].tolist() == [1, 0, 0, 1, 0, 1]
    assert r["matched_id"].tolist() == [100.0 + i for i in keep]
    assert np.array_equal(r["matched_3d"], cur["point_3d"][keep]) and np.array_equal(r["matched_2d_cur"], cur["point_2d_uv"][keep])
    assert np.array_equal(r["matched_2d_old"], okp[[0, 2, 3]]) and np.array_equal(r["matched_2d_old_norm"], onr[[0, 2, 3]])
