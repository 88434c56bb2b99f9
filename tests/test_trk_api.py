"""Tracker session (vpl_trk_*), the part that needs no GPU: the symbols are declared and exported, null arguments are
refused before any device is touched, and the ctypes structures have the sizes the header implies."""
import ctypes as C
import os
import re

import vplines_slam_amd as v

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vpl_trk_default_options", "vpl_trk_create", "vpl_trk_destroy", "vpl_trk_reset", "vpl_trk_frame", "vpl_trk_get_frame",
         "vpl_trk_debug_ids"]
VPL_E_INVALID = -1


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "vplines_frontend.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = v.load_hip_library()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), "not declared: " + n
        assert hasattr(lib, n), "missing export: " + n
    assert "typedef struct vpl_trk_options" in text and "typedef struct vpl_trk_result" in text
    assert v.TrackerSession is v.frontend.TrackerSession


def test_null_arguments_are_refused_without_a_device():
    lib = v.load_hip_library()
    v.frontend._bind(lib)
    opt = v.default_tracker_options()
    h = C.c_void_p()
    assert lib.vpl_trk_create(C.byref(h), None, 1, C.byref(opt)) == VPL_E_INVALID and not h.value
    assert lib.vpl_trk_create(None, None, 1, C.byref(opt)) == VPL_E_INVALID
    assert lib.vpl_trk_frame(None, None, None, None, None, None) == VPL_E_INVALID
    assert lib.vpl_trk_reset(None, 0) == VPL_E_INVALID
    assert lib.vpl_trk_get_frame(None, 0, None, None, None, None, None, None, None) == VPL_E_INVALID
    cnt = C.c_int(0)
    assert lib.vpl_trk_debug_ids(None, 0, None, 0, None, None, 0, None, 0, 0, C.byref(cnt), None, None, None, None, None) == VPL_E_INVALID
    lib.vpl_trk_destroy(None)   # a no-op


def test_struct_sizes_and_defaults_match_the_header():
    # vpl_edline_param: 6 x 4 bytes + double = 32; vpl_match_param: 10 x 4 = 40
    assert C.sizeof(v.frontend.EdlineParam) == 32 and C.sizeof(v.frontend.MatchParam) == 40
    # ed | match | max_h, max_v, equalize (12, then 4 of padding before the double) | clip_limit | tiles | K_
    assert C.sizeof(v.TrackerOptions) == 32 + 40 + 12 + 4 + 8 + 8 + 16
    assert v.TrackerOptions.clip_limit.offset == 88 and v.TrackerOptions.fx.offset == 104
    # 7 ints (28, padded to 32) | 9 doubles | int (padded to 8)
    assert C.sizeof(v.TrackerResult) == 32 + 72 + 8
    assert v.TrackerResult.vps.offset == 32 and v.TrackerResult.allfeature_cnt.offset == 104
    o = v.default_tracker_options()
    assert (o.ed.ksize, o.ed.scanIntervals, o.ed.minLineLen, o.ed.lineFitErrThreshold) == (5, 2, 35, 1.8)
    assert (o.match.step, o.match.illumination_adapt, o.match.topological_filter) == (10, 1, 1)
    assert (o.max_h_lines, o.max_v_lines, o.equalize, o.clip_limit, o.tiles_x, o.tiles_y) == (25, 25, 1, 3.0, 8, 8)
    assert (o.fx, o.fy, o.cx, o.cy) == (1.0, 1.0, 0.0, 0.0)
