"""The LDS layouts of the step kernels (csrc/ba_step_layout.h): one description for the host, which sizes every dispatch of k_step,
k_schur, k_chol, k_back and k_solve and decides which capacities a context accepts, and the device, whose bodies take every pointer
from it.  The header is plain C++; tests/native/step_layout_check.cpp walks every capacity and both tile counts under the address
and undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_step_layout_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "step_layout_check")
    # (ba_pack.h, for max_schur_ksteps, reaches ba_types.h, whose helpers carry the HIP function attributes)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-D__host__=", "-D__device__=",
                           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "step_layout_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "step layout ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
