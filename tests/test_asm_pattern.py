"""The static tables of k_lin's assembly of the packed camera Hessian (csrc/ba_asm_pattern.h): the entries a fast-path window's
factors can fill are stored for every window, the others only for windows of the general path, and every reader counts on zeros
there.  The header is plain C++; tests/native/asm_pattern_check.cpp checks the partition, its agreement with the list k_schur's
Cauchy pass walks, and every prior block table a fast-path window can carry (2^13 of them), under the address and
undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_asm_pattern_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "asm_pattern_check")
    # (ba_types.h's helpers carry the HIP function attributes)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-D__host__=", "-D__device__=",
                           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "asm_pattern_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "asm pattern ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
