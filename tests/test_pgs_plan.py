"""The host bookkeeping of the pose-graph session (csrc/pgs_plan.h) and the node flags of a graph of several sequences
(csrc/pg_plan.h).  The headers are plain C++; tests/native/pgs_plan_check.cpp runs random scripts of add / load / loop / optimise /
reset against a naive model under the address and undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_pgs_plan_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pgs_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "pgs_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "pgs plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
