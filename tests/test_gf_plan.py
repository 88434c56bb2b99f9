"""The plan of a global-fusion chain (csrc/gf_plan.h): separators, segments and the workspace layout, one description for the host
and the device.  The header is plain C++; tests/native/gf_plan_check.cpp walks every n <= 200 at S = 2..9 and the default under the
address and undefined-behaviour sanitizers (no GPU).  vpl_gf_debug_plan hands the same plan out."""
import os
import subprocess

import numpy as np

import vplines_slam_amd as v

import gf_ref


def test_gf_plan_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "gf_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "gf_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "gf plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_debug_plan_is_the_plan_of_the_restatement():
    for n in (1, 2, 3, 4, 5, 8, 9, 41, 131, 200):
        for S in (0, 2, 4, 7, 64, 300):
            p = v.gf_debug_plan(n, S)
            seps, segs = gf_ref.plan(n, S if S else gf_ref.DEFAULT_SEGMENT)
            assert list(p["sep_node"]) == seps and [tuple(b) for b in p["seg_bounds"]] == segs, (n, S)
    assert v.gf_debug_plan(5, 1) == -1 and v.gf_debug_plan(0, 4) == -1 and v.gf_debug_plan(5, -3) == -1
    assert v.gf_debug_plan(v.capi.GF_MAX_NODES + 1, 4) == -4
    big = v.gf_debug_plan(v.capi.GF_MAX_NODES, 2)
    assert len(big["sep_node"]) == v.capi.GF_MAX_NODES // 2 and np.array_equal(big["sep_node"][:3], [1, 3, 5])
