"""The IMU form of the keyframe session (include/vplines_ba.h, "IMU samples in"): the new structs of capi.py have the size their
field lists imply, every new entry point is exported by the built library and bound on Session.  No device call."""
import ctypes as C
import os
import re

import vplines_slam_amd as v

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vpl_odo_enable_imu": "enable_imu", "vpl_odo_set_imu": "set_imu", "vpl_odo_advance_imu": "advance_imu",
       "vpl_odo_keyframe_imu": "keyframe_imu", "vpl_odo_get_preint": "get_preint"}


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vplines_ba.h")).read(), flags=re.S)


def test_new_struct_sizes_match_their_field_lists():
    # vpl_odo_imu_frame: int + pointer, then twice (int, two pointers), natural alignment; vpl_odo_imu_out: 7 + 9 + 2 doubles
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(v.capi.OdoImuFrame) == 3 * p + 5 * p
    assert [f for f, _ in v.capi.OdoImuFrame._fields_] == ["n_samples", "samples", "n_points", "point_id", "point_obs", "n_lines", "line_id", "line_obs"]
    assert C.sizeof(v.capi.OdoImuOut) == 8 * (7 + 9 + 2)
    assert v.capi.OdoImuOut.sum_dt.offset == 8 * 16
    # the header declares the same members in the same order
    text = header_text()
    body = re.search(r"typedef struct vpl_odo_imu_frame \{(.*?)\} vpl_odo_imu_frame;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in v.capi.OdoImuFrame._fields_]
    body = re.search(r"typedef struct vpl_odo_imu_out \{(.*?)\} vpl_odo_imu_out;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\[(\d+)\]", body) == [("pose", "7"), ("speed_bias", "9"), ("sum_dt", "2")]
    # what existing callers rely on did not move
    assert C.sizeof(v.capi.OdoFrame) == 8 * 16 + C.sizeof(v.capi.Preintegration) + 2 * 3 * p
    assert C.sizeof(v.capi.OdoResult) == 8 * (77 + 99 + 7) + 2 * C.sizeof(v.capi.SolveReport) + 4 * 5 + 4


def test_every_new_odo_entry_point_is_exported_and_bound():
    lib = v.load_hip_library()
    declared = set(re.findall(r"\b(vpl_odo_[a-z0-9_]+)\s*\(", header_text()))
    assert set(NEW) <= declared, sorted(set(NEW) - declared)
    for name, method in NEW.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p, name
        assert callable(getattr(v.Session, method)), method
    # every vpl_odo_* function of the header, old or new, is exported
    for name in declared:
        assert hasattr(lib, name), "missing export: " + name
    assert v.ImuFrame is v.capi.ImuFrame and v.OdoImuOut is v.capi.OdoImuOut
    # a NULL session is refused by every new entry point without touching a device
    assert lib.vpl_odo_enable_imu(None, 4) == -1
    assert lib.vpl_odo_set_imu(None, 0, 1, None, None, None) == -1
    assert lib.vpl_odo_advance_imu(None, None, None, None) == -1
    assert lib.vpl_odo_keyframe_imu(None, None, None, None, None) == -1
    assert lib.vpl_odo_get_preint(None, 0, None) == -1
