"""k_marg's LDS layout (csrc/ba_marg_layout.h): one description for the host, which sizes the dispatch, and the device, which
takes every pointer from it.  The header is plain C++; tests/native/marg_layout_check.cpp walks every kept size and both forms
of the kernel under the address and undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_marg_layout_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "marg_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "marg_layout_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "marg layout ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
