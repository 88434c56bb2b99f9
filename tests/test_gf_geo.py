"""vpl_gf_local_cartesian (host only; replaces GPS2XYZ): WGS84 geodetic -> ECEF -> east, north, up, against the same closed form in
long double (tests/gf_ref.py).  Points up to 50 km from the origin, at the equator, at mid-latitude and at 89 degrees, within
max(32 |x64 - x80|, 1e-12 |ECEF|_inf), x64 the restatement in float64; the origin maps to 0."""
import numpy as np
import pytest

import vplines_slam_amd as v

import gf_ref

ORIGINS = {"equator": (0.0, 103.8, 15.0), "mid_latitude": (22.3364, 114.2655, 120.0), "near_pole": (89.0, -45.0, 5.0),
           "south_west": (-33.9, -70.6, 560.0)}


@pytest.mark.parametrize("name", list(ORIGINS))
def test_local_cartesian_against_long_double(name):
    lat0, lon0, h0 = ORIGINS[name]
    rng = np.random.default_rng(3)
    # offsets of up to 50 km: a degree of latitude is about 111 km; of longitude, that times cos(latitude)
    dlat = rng.uniform(-0.31, 0.31, 40)
    dlon = rng.uniform(-0.31, 0.31, 40) / max(np.cos(np.radians(lat0)), 0.02)
    lla = np.stack([np.clip(lat0 + dlat, -90, 90), lon0 + dlon, h0 + rng.uniform(-200, 3000, 40)], axis=1)
    lla[0] = (lat0, lon0, h0)
    got = v.local_cartesian(lat0, lon0, h0, lla)
    x64, _ = gf_ref.local_cartesian(lat0, lon0, h0, lla, np.float64)
    x80, ecef = gf_ref.local_cartesian(lat0, lon0, h0, lla, np.longdouble)
    assert np.abs(got[0]).max() == 0.0                                  # the origin
    far = float(np.linalg.norm(np.asarray(x80, np.float64), axis=1).max())
    assert 20e3 < far < 50e3, far
    bar = max(32 * float(np.abs(x64 - x80).max()), 1e-12 * float(np.abs(ecef).max()))
    err = float(np.abs(got.astype(np.longdouble) - x80).max())
    print(name, "error %.3g m, bar %.3g m, farthest point %.0f m" % (err, bar, far))
    assert err <= bar


def test_axes_and_refusals():
    # a step north, east and up from a mid-latitude origin lands on the matching axis
    lat0, lon0, h0 = ORIGINS["mid_latitude"]
    xyz = v.local_cartesian(lat0, lon0, h0, [[lat0 + 1e-4, lon0, h0], [lat0, lon0 + 1e-4, h0], [lat0, lon0, h0 + 10.0]])
    assert xyz[0, 1] > 10 and abs(xyz[0, 0]) < 1e-3 and xyz[1, 0] > 9 and abs(xyz[1, 1]) < 1e-3
    assert abs(xyz[2, 2] - 10.0) < 1e-8 and np.abs(xyz[2, :2]).max() < 1e-8
    assert len(v.local_cartesian(0, 0, 0, np.zeros((0, 3)))) == 0
    lib = v.load_hip_library()
    assert lib.vpl_gf_local_cartesian(0.0, 0.0, 0.0, 1, None, None) == -1
    assert lib.vpl_gf_local_cartesian(0.0, 0.0, 0.0, -1, None, None) == -1
