"""k_trk_ids, the tracker session's id / t_cnt / quota kernel, alone (vpl_trk_debug_ids) against the host function
vpl_line_track_ids on the same inputs."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as o
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    ctx = v.frontend.FrontendContext(device=0, max_images=1, width=64, height=64, max_lines=16)
    yield ctx
    ctx.close()


def device_track_ids(fe, ends, id_prev, tcnt_prev, p2n, max_h, max_v, cnt):
    ends = np.ascontiguousarray(ends, np.float32).reshape(-1, 4)
    n_new = len(ends)
    idp, tcp, p2n = (np.ascontiguousarray(a, np.int32) for a in (id_prev, tcnt_prev, p2n))
    keep, ids, tc, vert = (np.full(max(n_new, 1), -7, np.int32) for _ in range(4))
    c, nvert = C.c_int(cnt), C.c_int(0)
    ip = C.POINTER(C.c_int)
    n = fe.lib.vpl_trk_debug_ids(fe.h, n_new, ends.ctypes.data_as(C.POINTER(C.c_float)), len(p2n), idp.ctypes.data_as(ip),
                                 tcp.ctypes.data_as(ip), len(tcp), p2n.ctypes.data_as(ip), max_h, max_v, C.byref(c),
                                 keep.ctypes.data_as(ip), ids.ctypes.data_as(ip), tc.ctypes.data_as(ip), vert.ctypes.data_as(ip),
                                 C.byref(nvert))
    assert n >= 0, fe.lib.vpl_fe_last_error(fe.h)
    return keep[:n].copy(), ids[:n].copy(), tc[:n_new].copy(), c.value, vert[:nvert.value].copy()


def agree(fe, ends, id_prev, tcnt_prev, p2n, max_h, max_v, cnt):
    hip = v.load_hip_library()
    want = o.track_ids(ends, id_prev, tcnt_prev, p2n, max_h, max_v, cnt, lib=hip, fn="vpl_line_track_ids", with_vertical=True)
    got = device_track_ids(fe, ends, id_prev, tcnt_prev, p2n, max_h, max_v, cnt)
    for name, x, y in zip(("keep", "ids", "t_cnt", "allfeature_cnt", "vertical"), want, got):
        assert np.array_equal(x, y), name
    return want


def test_id_kernel_equals_the_host_function_on_random_lists(fe):
    """The inputs of test_track_ids_oracle_product_and_python_agree (n_new 0..60, n_prev 0..50, matches with 0, duplicates and
    out-of-range values, a t_cnt vector shorter and longer than n_new, quotas 0..40, the vertical segment and the 45 degree
    border case): keep, ids, t_cnt, the vertical list and the counter are equal to vpl_line_track_ids, element for element.

    Not tested, by construction: a segment whose angle lies within an ulp (of float) of 3.14 / 4 or 3 * 3.14 / 4 could be
    classed differently if the device's atan2 differs from glibc's atan2f by an ulp.  None of these inputs is such a case: the
    "45 degree" segment has the angle 0.7853986, 4e-4 away from 3.14 / 4 = 0.785."""
    rng = np.random.default_rng(2)
    kept = 0
    for trial in range(60):
        n_new, n_prev = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        ends = rng.uniform(0, 700, (n_new, 4)).astype(np.float32)
        if n_new > 3:
            ends[1, 2] = ends[1, 0]                              # a vertical segment (x2 == x1)
            ends[2] = [10, 10, 20, 20.00001]                     # right at the 45 degree border
        id_prev = rng.integers(0, 1000, n_prev).astype(np.int32)
        tcnt_prev = rng.integers(0, 9, int(rng.integers(0, 70))).astype(np.int32)
        p2n = rng.integers(-1, max(n_new, 1) + 3, n_prev).astype(np.int32)      # includes 0 (ignored) and out-of-range
        max_h, max_v = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        kept += len(agree(fe, ends, id_prev, tcnt_prev, p2n, max_h, max_v, 500 + trial)[0])
    assert kept > 500


def test_more_lines_than_threads_quota_zero_and_no_previous_line(fe):
    rng = np.random.default_rng(5)
    # 300 detections on a block of 256 threads; some previous ids are -1, which the host function reads as "no id"
    n_new, n_prev = 300, 220
    ends = rng.uniform(0, 700, (n_new, 4)).astype(np.float32)
    id_prev = rng.integers(0, 5000, n_prev).astype(np.int32)
    id_prev[::17] = -1
    p2n = rng.integers(-1, n_new + 3, n_prev).astype(np.int32)
    tcnt_prev = rng.integers(0, 9, 280).astype(np.int32)
    keep, ids, tc, cnt, vert = agree(fe, ends, id_prev, tcnt_prev, p2n, 60, 70, 9000)
    assert len(keep) > 130 and keep.max() > 256 and tc[257:].any() and len(vert) > 40
    # quotas 0 / 0: only tracked lines are kept
    keep0, ids0, _, cnt0, vert0 = agree(fe, ends, id_prev, tcnt_prev, p2n, 0, 0, 9000)
    assert 0 < len(keep0) < len(keep) and cnt0 == cnt and np.array_equal(vert0, vert) and (ids0 < 9000).all()
    # no previous line: everything is fresh, the quota cuts
    keepn, idsn, tcn, cntn, _ = agree(fe, ends[:50], [], [], [], 10, 12, 40)
    assert len(keepn) == 22 and not tcn.any() and cntn == 90
    # the documented quirks: a match to detection 0 is dropped, tracked lines are never cut by the quota, later match wins
    e4 = np.array([[0, 0, 100, 0]] * 4, np.float32)
    keep, ids, tc, cnt, _ = agree(fe, e4, [7, 8, 9, 10], [5, 5, 5, 5], [0, 1, 3, 3], 0, 0, 100)
    assert list(keep) == [1, 3] and list(ids) == [8, 10] and list(tc) == [0, 6, 0, 6] and cnt == 102
    # an empty frame
    agree(fe, np.zeros((0, 4), np.float32), [3, 4], [1], [0, 1], 5, 5, 11)
