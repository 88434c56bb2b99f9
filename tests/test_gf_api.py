"""The global-fusion structs of capi.py against include/vplines_ba.h (sizes: ints and doubles only, natural alignment) and the
default options against the restatement's (no GPU)."""
import ctypes as C

import vplines_slam_amd as v

import gf_ref


def test_struct_sizes_match_the_header():
    assert C.sizeof(v.capi.GfOptions) == 4 * 4 + 12 * 8
    assert C.sizeof(v.capi.CGfInput) == 2 * 4 + 5 * 8
    assert C.sizeof(v.capi.CGfResult) == 6 * 4 + 8 * (2 + 16) + 8
    assert v.capi.GF_MAX_NODES == 65536
    assert (v.capi.GF_NO_CONVERGENCE, v.capi.GF_CONVERGENCE, v.capi.GF_FAILURE) == (gf_ref.NO_CONVERGENCE, gf_ref.CONVERGENCE, gf_ref.FAILURE)


def test_default_options_equal_the_restatements():
    o = v.default_gf_options()
    ref = gf_ref.default_options()
    assert set(ref) == {f for f, _ in v.capi.GfOptions._fields_}
    for f, _ in v.capi.GfOptions._fields_:
        assert getattr(o, f) == ref[f], f
    assert v.default_gf_options(segment=4, huber_delta=0.5).segment == 4
