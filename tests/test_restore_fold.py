"""The pending state restore of a context (csrc/ba_restore.h): vpl_ba_reset_state enqueues nothing, the next solve restores
inside k_prep and every other call flushes.  The decision is a host-only function; tests/native/restore_fold_check.cpp drives
it through the call sequences of the library under the address and undefined-behaviour sanitizers (no GPU)."""
import os
import subprocess


def test_restore_decision_table_under_the_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "restore_fold_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-I" + os.path.join(root, "vplines-slam_amd", "csrc"),
                           os.path.join(root, "tests", "native", "restore_fold_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, "11"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "restore decision table ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
