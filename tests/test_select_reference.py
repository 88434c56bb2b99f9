"""The model of the feature selector (tests/select_ref.py) against closed forms, its float64 and long double runs on every scene
of tests/select_inputs.py, the host-only id book (vpl_sel_debug_book) against the restatement's, the struct sizes and the id
book's header under the sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import select_inputs as si
import select_ref as ref
import vplines_slam_amd as v

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cov_imu_inverse_is_its_block_form():
    """the general inverse the restatement takes against the closed form the device uses: [[a I, b I, 0], [b I, c I, 0], [0, 0, e I]]"""
    for dt in (np.float64, np.longdouble):
        for n, d in ((10, 0.005), (2, 0.025), (40, 0.0025)):
            W, _ = ref.imu_matrices(dt, np.array([1, 0, 0, 0], dtype=dt), np.array([1, 0, 0, 0], dtype=dt), n, d, 0.08, 0.0004)
            Wc = ref.cov_imu_inverse_closed(dt, n, d, 0.08, 0.0004)
            assert np.abs(W - Wc).max() <= 1e-9 * np.abs(Wc).max(), (dt, n)
            assert np.abs(W @ ref.cov_imu(dt, n, d, 0.08, 0.0004) - np.eye(9)).max() < 1e-8


def test_cov_imu_of_one_sample_is_singular():
    """n_imu = 1: CCt_11 = 1/4, CCt_12 = 1/2 and the position / velocity block has determinant a c - b^2 = 0 exactly -- the
    reference's covImu.inverse() is then not a number that can be compared; a property of the reference"""
    cov = ref.cov_imu(np.longdouble, 1, 0.05, 0.08, 0.0004)
    a, b, c = cov[0, 0], cov[0, 3], cov[3, 3]
    assert abs(a * c - b * b) <= 4 * np.finfo(np.longdouble).eps * a * c


def test_omega_is_positive_definite_and_delta_is_blind_to_translation():
    rng = np.random.default_rng(0)
    for name in ("12 candidates", "own horizon", "behind"):
        r = si.reference(name)
        for run in (r["r64"], r["r80"]):
            Om = np.array(run["omega"], dtype=np.float64)
            assert np.abs(Om - Om.T).max() <= 1e-9 * np.abs(Om).max()
            assert np.linalg.eigvalsh((Om + Om.T) / 2).min() > 0
            assert np.all(np.isfinite(ref.logdet_chol(run["omega"][None])))
            for D in list(run["deltas"].values()) + run["used"]:
                Df = np.array(D, dtype=np.float64)
                scale = np.abs(Df).max()
                assert np.abs(Df - Df.T).max() <= 1e-12 * scale
                assert np.linalg.eigvalsh((Df + Df.T) / 2).min() >= -1e-12 * scale
                t = np.zeros(ref.N45)
                d = rng.normal(size=3)
                for i in range(1, 5):
                    t[9 * i:9 * i + 3] = d               # all four positions moved along one direction
                assert np.abs(Df @ t).max() <= 1e-12 * scale * np.abs(d).max()
                z = np.ones(ref.N45, dtype=bool)
                z[ref.POS12] = False
                assert not Df[z].any() and not Df[:, z].any()      # nothing outside the 12 position dimensions


def test_upper_bound_is_above_the_value():
    for name in si.SCENES:
        r = si.reference(name) if name not in si.DEGENERATE else None
        for run in ((r["r64"], r["r80"]) if r else ()):
            for cand, ub, f, _ in run["rounds"]:
                ok = np.isfinite(np.asarray(f, dtype=np.float64))
                assert np.all(np.asarray(ub)[ok] >= np.asarray(f)[ok]), name


def test_the_two_precisions_agree_on_every_scene():
    """si.reference asserts the selection bar (no scene may be left out of it but the singular one); here: the same ids, f and
    Omega_kkH close in the two precisions"""
    for name in si.SCENES:
        if name in si.DEGENERATE:
            continue
        r = si.reference(name)
        r64, r80 = r["r64"], r["r80"]
        assert r64["ids"] == r80["ids"]
        if len(r64["f"]):
            assert np.abs(r64["f"] - r80["f"]).max() < 1e-6
        assert np.abs(r64["omega"] - r80["omega"]).max() <= 1e-9 * np.abs(r80["omega"]).max()
        s = r["scene"]
        assert len(r64["ids"]) <= min(s.kappa, len(s.new_id))
    assert si.reference("2 identical")["r64"]["ids"] == [1001, 1000]          # the higher id first, then the lower
    assert si.reference("huge variances")["r64"]["ids"] == [] and si.reference("kappa 0")["r64"]["ids"] == []
    assert si.reference("invisible")["r64"]["invisible"] == [1001]
    assert len(si.reference("kappa above")["r64"]["ids"]) == 5


def _script():
    """a first image, an uninitialised stretch below init_thresh, ids that disappear and come back, kappa = 0"""
    images = [list(range(1, 9)),                       # the first image: everything is taken and tracked
              [1, 2, 3, 9, 10],                        # not initialised, 3 tracked present < init_thresh: the old ids come in, the new do not
              [2, 3, 11, 12, 13],                      # still not initialised
              [1, 3, 5, 14, 15, 16, 17],               # initialised: 1 and 5 are back; kappa = 6 - 3
              [3, 14, 15, 18, 19, 20, 21, 22],         # 14 was selected, 15 was not (it stays out for good)
              [1, 2, 3, 5, 14, 18, 23, 24],            # six tracked ids present: kappa = 0
              [30, 31]]                                # nothing known: kappa = max_features
    initialized = [False, False, False, True, True, True, True]
    offers = [[], [9], [11], [16, 14, 99, 17, 15], [20, 18], [23], [31, 30]]
    return images, initialized, offers


def test_id_book_against_the_restatement():
    images, initialized, offers = _script()
    got = v.select_debug_book(6, 4, images, initialized, offers)
    assert isinstance(got, dict), got
    book = ref.Book(6, 4)
    for s, (img, init, off) in enumerate(zip(images, initialized, offers)):
        image, new, subset, kappa = book.split(img)
        sel = [i for i in off if i in new][:kappa] if init else []
        out = book.finish(image, new, subset, init, sel)
        assert got["n_new"][s] == len(new) and got["kappa"][s] == kappa and got["last_id"][s] == book.last_id, s
        assert list(got["selected"][s]) == sel and list(got["out"][s]) == out and got["n_tracked"][s] == len(book.tracked), s
    assert list(got["tracked"]) == book.tracked
    assert list(got["kappa"]) == [6, 3, 4, 3, 4, 0, 6]
    assert list(got["out"][0]) == list(range(1, 9)) and list(got["out"][1]) == [1, 2, 3] and list(got["selected"][3]) == [16, 14, 17]
    assert list(got["out"][5]) == [1, 2, 3, 5, 14, 18] and len(got["selected"][5]) == 0


def test_struct_sizes():
    assert C.sizeof(v.capi.SelectParams) == 8 * 2 + 4 * 4 + 8 * 8 + 8 * 4 + 8 * 3
    assert C.sizeof(v.capi.CSelectInput) == 8 * 33 + 4 * 2 + 8 + (4 + 4) + 8 * 4 + (4 + 4) + 8 * 2 + (4 + 4) + 8
    assert C.sizeof(v.capi.SelectResult) == 16
    assert C.sizeof(v.capi.CSelectFrame) == 8 * 19 + 8 + (4 + 4) + 8 + (4 + 4) + 8 * 4
    assert C.sizeof(v.capi.OdoSelectResult) == 16 + 4 * 6


def test_book_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sel_book_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vplines-slam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sel_book_check.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "sel book ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
