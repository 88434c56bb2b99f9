"""The prior rule of a context (vpl_ba_set_prior_rule, include/vplines_ba.h): exported by the library, its two constants in
the header and in the Python bindings.  No compute call: runs without a GPU."""
import ctypes as C
import os
import re

import vplines_slam_amd as v

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_setter():
    lib = v.load_hip_library()
    assert hasattr(lib, "vpl_ba_set_prior_rule")


def test_header_defines_both_rules():
    text = open(os.path.join(ROOT, "include", "vplines_ba.h")).read()
    consts = dict(re.findall(r"#define\s+(VPL_PRIOR_[A-Z_]+)\s+(-?\d+)", text))
    assert consts == {"VPL_PRIOR_PIVOTED_CHOLESKY": "0", "VPL_PRIOR_EIGEN": "1"}
    assert re.search(r"int\s+vpl_ba_set_prior_rule\s*\(\s*vpl_ctx\s*\*\s*ctx\s*,\s*int\s+rule\s*\)\s*;", text)


def test_python_bindings():
    assert v.capi.PRIOR_PIVOTED_CHOLESKY == 0 and v.capi.PRIOR_EIGEN == 1
    assert v.PRIOR_PIVOTED_CHOLESKY == 0 and v.PRIOR_EIGEN == 1
    assert callable(getattr(v.Context, "set_prior_rule", None))


def test_null_context_is_refused():
    lib = v.load_hip_library()
    lib.vpl_ba_set_prior_rule.argtypes = [C.c_void_p, C.c_int]
    for rule in (0, 1, 2, -1):
        assert lib.vpl_ba_set_prior_rule(None, rule) == -1   # VPL_E_INVALID, no device touched
