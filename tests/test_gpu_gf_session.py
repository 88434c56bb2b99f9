"""The global-fusion session (vpl_gf_create .. vpl_gf_destroy): 30 poses fed one at a time, a fix on every fifth and an optimize
after each fix.  Its results equal, byte for byte, the chain of vpl_gf_optimize_batch calls that carries the global poses and
WGPS_T_WVIO forward by hand; input_odom's returned pose is WGPS_T_WVIO applied on the host; the capacity and timestamp refusals."""
import ctypes as C

import numpy as np
import pytest

import vplines_slam_amd as v

import gf_inputs
import gf_ref

pytestmark = pytest.mark.gpu

N = 30


def test_session_equals_the_chain_of_batch_calls(gpu_ctx):
    g = gf_inputs.make_chain(N, range(0, N, 5), 41, turns=0.8)
    local, fixes = g["local"], dict(zip(g["gps_node"].tolist(), range(len(g["gps_node"]))))
    opt = v.default_gf_options(segment=4)
    T = np.eye(4)
    glob = np.zeros((0, 7))        # by hand: the global poses of the nodes so far
    nodes, xyz, acc = [], [], []
    runs = 0
    with v.GlobalFusionSession(gpu_ctx, 64) as s:
        s.input_gps(123.0, [1.0, 2.0, 3.0], 0.5)                      # no node has this time: stored, never used
        for k in range(N):
            t = 100.0 + 0.1 * k
            gp, gq = s.input_odom(t, local[k, :3], local[k, 3:])
            # the returned pose is WGPS_T_WVIO applied on the host
            R = T[:3, :3]
            assert np.abs(gp - (R.dot(local[k, :3]) + T[:3, 3])).max() <= 1e-12 * max(1.0, np.abs(gp).max())
            assert np.abs(gf_ref.qmat(gq) - R.dot(gf_ref.qmat(local[k, 3:]))).max() <= 1e-12
            glob = np.concatenate([glob, np.concatenate([gp, gq])[None]])
            if k not in fixes:
                continue
            e = fixes[k]
            s.input_gps(t, g["gps_xyz"][e], g["gps_accuracy"][e])
            nodes.append(k), xyz.append(g["gps_xyz"][e]), acc.append(g["gps_accuracy"][e])
            got = s.optimize(opt)
            want = gpu_ctx.global_fusion([v.GlobalFusionInput(local[:k + 1], glob, nodes, xyz, acc)], opt)[0]
            path = s.path(0, k + 1)
            assert got.head.status == want.status and got.pose is None
            assert got.data_head() == want.data_head(), k
            assert path.tobytes() == want.pose.tobytes(), k
            assert np.array_equal(s.path(k, 1)[0], want.pose[k])
            glob, T = want.pose.copy(), want.T
            runs += 1
        assert runs == 6 and want.iterations >= 1 and np.abs(T - np.eye(4)).max() > 1e-3
        # a fix that replaces an earlier one is seen by the next solve
        s.input_gps(100.0, g["gps_xyz"][0] + 0.3, 0.4)
        xyz[0], acc[0] = g["gps_xyz"][0] + 0.3, 0.4
        got = s.optimize(opt)
        want = gpu_ctx.global_fusion([v.GlobalFusionInput(local, glob, nodes, xyz, acc)], opt)[0]
        assert got.data_head() == want.data_head() and s.path(0, N).tobytes() == want.pose.tobytes()


def test_session_refusals(gpu_ctx):
    q = np.array([1.0, 0, 0, 0])
    with v.GlobalFusionSession(gpu_ctx, 3) as s:
        assert s.optimize(check=False) == -1                          # no node yet
        s.input_odom(1.0, [0, 0, 0], q)
        assert s.input_odom(1.0, [1, 0, 0], q, check=False) == -1     # the time does not increase
        assert s.input_odom(0.5, [1, 0, 0], q, check=False) == -1
        assert s.input_odom(2.0, [np.nan, 0, 0], q, check=False) == -1
        assert s.input_gps(1.0, [0, 0, 0], 0.0, check=False) == -1
        assert s.input_gps(1.0, [0, np.inf, 0], 1.0, check=False) == -1
        s.input_odom(2.0, [1, 0, 0], q)
        s.input_odom(3.0, [2, 0, 0], q)
        assert s.input_odom(4.0, [3, 0, 0], q, check=False) == -4     # max_nodes
        assert s.path(2, 2, check=False) == -1 and len(s.path(0, 3)) == 3
        assert s.optimize(v.default_gf_options(segment=1), check=False) == -1
        r = s.optimize()                                              # no fix: nothing moves
        assert r.iterations == 0 and np.array_equal(s.path(0, 3)[:, :3], [[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    lib = v.load_hip_library()
    h = C.c_void_p()
    assert lib.vpl_gf_create(gpu_ctx.h, 0, C.byref(h)) == -1 and lib.vpl_gf_create(gpu_ctx.h, v.capi.GF_MAX_NODES + 1, C.byref(h)) == -4
