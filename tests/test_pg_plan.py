"""The plan of a pose graph (csrc/pg_plan.h): the edge slots, the order in which a node gathers its incident edges, and the
workspace layout, one description for the host and the device.  The header is plain C++; tests/native/pg_plan_check.cpp walks every
n <= 70 with random loop sets under the address and undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_pg_plan_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pg_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "pg_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "pg plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
