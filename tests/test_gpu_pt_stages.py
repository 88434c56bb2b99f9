"""The point front-end's stage calls on the device against tests/pt_ref.py, bit for bit."""
import numpy as np
import pytest

import vplines_slam_amd as v

import pt_inputs

pytestmark = pytest.mark.gpu

VPL_E_CAPACITY = -4


def make_ctx(images, max_candidates=8192, max_corners=256):
    n, H, W = images.shape
    fe = v.frontend.FrontendContext(max_images=n, width=W, height=H, max_lines=64)
    fe.pt_reserve(max_candidates, max_corners)
    return fe


@pytest.mark.parametrize("name", ["full", "full_mask40", "crop160x120", "crop64x48_sparse_mask", "batch3_one_constant"])
def test_pt_detect_matches_the_reference_bit_for_bit(name):
    images, mc, md, masks = pt_inputs.detect_cases()[name]
    ref = pt_inputs.ref_detect_case(name)
    fe = make_ctx(images)
    try:
        got = fe.pt_detect(images, mc, md, masks)
        for i, ((c, s), (rc, rs, rtotal)) in enumerate(zip(got, ref)):
            eig, found = fe.pt_debug_detect(i)
            print(name, i, "corners", len(c), "ref", len(rc), "candidates", found, "ref", rtotal)
            assert found == rtotal
            assert c.shape == rc.shape and np.array_equal(c, rc), "corner list of image %d differs" % i
            assert np.array_equal(s.view(np.uint32), rs.view(np.uint32)), "scores of image %d differ in bits" % i
    finally:
        fe.close()
    if name == "full":
        assert len(ref[0][0]) == 150
    if name == "full_mask40":
        assert len(ref[0][0]) == 37
    if name == "crop64x48_sparse_mask":
        assert 0 < len(ref[0][0]) < mc[0]
    if name == "batch3_one_constant":
        assert len(ref[1][0]) == 0 and len(ref[0][0]) > 0 and len(ref[2][0]) > 0


def test_pt_detect_plane_matches_the_reference_bit_for_bit():
    """the cornerMinEigenVal plane itself, borders included, on a crop whose sizes are no multiple of the kernel's tile"""
    import pt_ref
    img = pt_inputs.crop(7, 123, 77, 75, 53)[None]
    fe = make_ctx(img)
    try:
        fe.pt_detect(img, 10, 5.0)
        eig, _ = fe.pt_debug_detect(0)
    finally:
        fe.close()
    ref = pt_ref.min_eig_plane(img[0])
    assert np.array_equal(eig.view(np.uint32), ref.view(np.uint32))


def test_pt_detect_refuses_a_candidate_list_that_overflows():
    images = pt_inputs.frames()[1:2]
    total = pt_inputs.ref_detect_case("full")[0][2]
    fe = make_ctx(images, max_candidates=total - 1)
    try:
        n, MC = 1, fe.pt_max_corners
        import ctypes as C
        corners = np.full((n, MC, 2), -7, np.float32)
        scores = np.full((n, MC), -7, np.float32)
        counts = np.full(n, -7, np.int32)
        mc, md = np.array([150], np.int32), np.array([30.0])
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        rc = fe.lib.vpl_pt_detect_batch(fe.h, n, images.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, mc.ctypes.data_as(ip),
                                        md.ctypes.data_as(C.POINTER(C.c_double)), corners.ctypes.data_as(fp),
                                        scores.ctypes.data_as(fp), counts.ctypes.data_as(ip))
        assert rc == VPL_E_CAPACITY
        assert str(total) in fe.lib.vpl_fe_last_error(fe.h).decode()
        assert (corners == -7).all() and (scores == -7).all() and (counts == -7).all()   # nothing truncated, nothing written
    finally:
        fe.close()
    # one more entry and the same frame passes
    fe = make_ctx(images, max_candidates=total)
    try:
        (c, s), = fe.pt_detect(images, 150, 30.0)
        rc_, rs_, _ = pt_inputs.ref_detect_case("full")[0]
        assert np.array_equal(c, rc_) and np.array_equal(s.view(np.uint32), rs_.view(np.uint32))
    finally:
        fe.close()


@pytest.mark.parametrize("name", ["7_points", "8_points", "150_points_30_outliers", "batch_of_2"])
def test_pt_reject_f_matches_the_reference_on_the_same_stream(name):
    import pt_ref
    case = pt_inputs.reject_cases()[name]
    cam = v.frontend.PointCamera(*pt_inputs.CAM)
    fe = v.frontend.FrontendContext(max_images=len(case), width=pt_inputs.W, height=pt_inputs.H, max_lines=64)
    fe.pt_reserve(max_points=160)
    try:
        got = fe.pt_reject_f([c for c, _, _ in case], [f for _, f, _ in case], cam, [s for _, _, s in case])
        again = fe.pt_reject_f([c for c, _, _ in case], [f for _, f, _ in case], cam, [s for _, _, s in case])
    finally:
        fe.close()
    for i, (cur, forw, seed) in enumerate(case):
        want = pt_ref.reject_f(cur, forw, pt_inputs.CAM, pt_inputs.W, pt_inputs.H,
                               lambda N: v.relpose_debug_plan(seed, 0, N)["samples"])
        print(name, i, "kept", int(got[i].sum()), "of", len(cur), "reference", int(want.sum()))
        assert got[i].dtype == np.uint8 and np.array_equal(got[i], want)
        assert np.array_equal(got[i], again[i])
    if name == "7_points":
        assert got[0].tolist() == [1] * 7
    if name == "batch_of_2":
        # the same list under another seed alone: a list's mask does not depend on its neighbour
        fe = v.frontend.FrontendContext(max_images=1, width=pt_inputs.W, height=pt_inputs.H, max_lines=64)
        fe.pt_reserve(max_points=160)
        try:
            alone, = fe.pt_reject_f([case[1][0]], [case[1][1]], cam, [case[1][2]])
        finally:
            fe.close()
        assert np.array_equal(alone, got[1])


@pytest.mark.parametrize("name", ["frames_1_2_150_points", "crop160x120_3_levels", "borders_and_corners", "constant_patch",
                                  "batch_0_1_65_points"])
def test_pt_flow_matches_the_reference_bit_for_bit(name):
    images, pairs, pts = pt_inputs.flow_cases()[name]
    ref = pt_inputs.ref_flow_case(name)
    n, H, W = images.shape
    fe = v.frontend.FrontendContext(max_images=max(n, len(pairs)), width=W, height=H, max_lines=64)
    fe.pt_reserve(max_points=160)
    try:
        fe.upload(images)
        got = fe.pt_flow(pairs, pts)
    finally:
        fe.close()
    for i, ((nxt, st), (rn, rs)) in enumerate(zip(got, ref)):
        print(name, i, len(st), "points, tracked", int(st.sum()), "reference", int(rs.sum()),
              "positions that differ", int((nxt.view(np.uint32) != rn.view(np.uint32)).any(axis=1).sum()) if len(st) else 0)
        assert np.array_equal(st, rs), "status of pair %d differs" % i
        assert np.array_equal(nxt.view(np.uint32), rn.view(np.uint32)), "next_pts of pair %d differ in bits" % i


def test_pt_stage_refusals_leave_the_context_usable():
    VPL_E_INVALID = -1
    import ctypes as C
    images, mc, md, masks = pt_inputs.detect_cases()["crop160x120"]
    fe = v.frontend.FrontendContext(max_images=1, width=160, height=120, max_lines=64)
    ip, fp, u8 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    try:
        # nothing reserved yet
        one, dist = np.array([10], np.int32), np.array([5.0])
        out_c, out_s, out_n = np.zeros((1, 64, 2), np.float32), np.zeros((1, 64), np.float32), np.zeros(1, np.int32)

        def detect(n, corners, distance):
            return fe.lib.vpl_pt_detect_batch(fe.h, n, images.ctypes.data_as(u8), None, None, corners.ctypes.data_as(ip),
                                              distance.ctypes.data_as(C.POINTER(C.c_double)), out_c.ctypes.data_as(fp),
                                              out_s.ctypes.data_as(fp), out_n.ctypes.data_as(ip))
        assert detect(1, one, dist) == VPL_E_INVALID
        assert fe.lib.vpl_pt_reserve(fe.h, 16385, 64, 64) == VPL_E_CAPACITY
        assert fe.lib.vpl_pt_reserve(fe.h, 4096, 2049, 64) == VPL_E_CAPACITY
        assert fe.lib.vpl_pt_reserve(fe.h, 4096, 64, 1025) == VPL_E_CAPACITY
        fe.pt_reserve(4096, 64, 64)
        assert fe.lib.vpl_pt_reserve(fe.h, 4096, 64, 64) == VPL_E_INVALID          # twice
        assert detect(2, np.array([10, 10], np.int32), np.array([5.0, 5.0])) == VPL_E_CAPACITY     # more images than slots
        assert detect(1, np.array([0], np.int32), dist) == VPL_E_INVALID            # max_corners below 1
        assert detect(1, np.array([65], np.int32), dist) == VPL_E_CAPACITY          # above the reserved row length
        assert detect(1, one, np.array([-1.0])) == VPL_E_INVALID
        assert detect(1, one, np.array([np.nan])) == VPL_E_INVALID
        # a list longer than max_points
        long_list = [np.zeros((65, 2), np.float32)]
        with pytest.raises(RuntimeError, match="max_points"):
            fe.pt_reject_f(long_list, long_list, v.frontend.PointCamera(*pt_inputs.CAM), [1])
        fe.upload(images)
        with pytest.raises(RuntimeError, match="max_points"):
            fe.pt_flow([(0, 0)], long_list)
        with pytest.raises(RuntimeError, match="not in the context"):
            fe.pt_flow([(0, 1)], [np.zeros((1, 2), np.float32)])
        # and the context still works
        (c, s), = fe.pt_detect(images, 64, md)             # the greedy pass stopped at 64 keeps the first 64 of a longer run
        (rc, rs, _), = pt_inputs.ref_detect_case("crop160x120")
        assert len(c) == 64 and np.array_equal(c, rc[:64]) and np.array_equal(s.view(np.uint32), rs.view(np.uint32)[:64])
    finally:
        fe.close()
    # a frame no larger than the 21 x 21 window: detection works, tracking is refused
    tiny = pt_inputs.crop(1, 300, 200, 20, 20)[None]
    fe = v.frontend.FrontendContext(max_images=1, width=20, height=20, max_lines=64)
    try:
        fe.pt_reserve(1024, 16, 16)
        (c, s), = fe.pt_detect(tiny, 5, 3.0)
        import pt_ref
        rc, rs = pt_ref.detect(tiny[0], 5, 3.0)
        assert np.array_equal(c, rc) and np.array_equal(s.view(np.uint32), rs.view(np.uint32))
        fe.upload(tiny)
        with pytest.raises(RuntimeError, match="window"):
            fe.pt_flow([(0, 0)], [np.array([[10, 10]], np.float32)])
    finally:
        fe.close()
