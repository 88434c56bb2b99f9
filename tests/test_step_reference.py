"""The long-double restatement of one trust-region iteration (step_ref.py) against the oracle, on the CPU: the reference has
to be right before test_gpu_step_kernels.py lets it judge a kernel.  Per case the oracle runs ONE iteration without
marginalisation; the window it hands back must be x0 [+] delta_ref carried through the gauge fix and the Pluecker conversion.

Bounds: the solve A y = b of a step is backward stable in double, so the oracle's step is within the standard forward bound
8 eps64 cond2(A_ref) |delta_ref| of the reference's, taken per block class (translations, rotations, speed/bias, extrinsic,
inverse depths, lines), plus 8 eps64 |x| for the arithmetic of the update itself.  The gauge fix then rotates every pose by the
yaw error of frame 0 about frame 0 and the lines with it; the bounds of the handed-back quantities below are those class
bounds pushed through that map.  Nothing here is measured on the code under test.

The same cases also have to satisfy what the GPU tests rely on: both Huber regimes among the visual residual blocks, none of
them within 1e-9 of the threshold (where rounding decides the branch), a first step that is accepted, on the Gauss-Newton
branch, at mu = 1e-8."""
import re

import numpy as np
import pytest

import oracle_api as o
import step_ref as sr

CASES = ["a", "b", "c", "d", "e", "f", "g", "i_ex", "i_tri"]
EPS = sr.EPS64


def _qdiff(a, b):
    """largest entry of a - b with the sign of every quaternion row chosen (q and -q are one rotation)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return max(min(np.abs(x - y).max(), np.abs(x + y).max()) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def oracle_runs():
    """case -> (window after the oracle's one iteration, report, the oracle's debug lines)"""
    return {}


def _oracle(case, cache, monkeypatch, capfd):
    if case not in cache:
        w, opt = sr.cases()[case]
        wc = w.copy()
        monkeypatch.setenv("ORC_DEBUG", "1")
        capfd.readouterr()
        _, rep = o.solve_window(wc, opt)
        cache[case] = (wc, rep, capfd.readouterr().err)
    return cache[case]


def test_the_cases_are_the_shapes_they_claim():
    c = sr.cases()
    shape = lambda k: (len(c[k][0].point_start), len(c[k][0].line_start))
    assert shape("a") == (0, 0) and shape("c") == (5, 1) and shape("d") == (37, 11) and shape("e") == (12, 6)
    b = c["b"][0]
    assert shape("b") == (1, 0) and list(b.point_start) == [0] and list(b.point_nobs) == [2]
    d = c["d"][0]
    assert len(set(d.point_nobs)) > 2 and len(set(d.line_nobs)) > 1 and d.point_nobs.max() <= 6       # ragged 6-frame tracks
    e = c["e"][0]
    assert sorted(set(e.point_start)) == list(range(8)) and (e.point_start + e.point_nobs).max() == 11
    assert any(e.point_start[p] + e.point_nobs[p] == 11 for p in range(12)) and any(e.point_start[p] + e.point_nobs[p] < 11 for p in range(12))
    assert e.line_nobs.max() == 11 and e.line_nobs.min() < 11
    f, g = c["f"][0], c["g"][0]
    assert 39 <= f.prior.n <= 75 and all(f.prior.block_frame[b] == 0 for b in range(f.prior.n_blocks) if f.prior.block_kind[b] == 1)
    assert any(g.prior.block_kind[b] == 1 and g.prior.block_frame[b] != 0 for b in range(g.prior.n_blocks))
    assert c["i_ex"][1].estimate_extrinsic == 0 and sr.Problem(*c["i_tri"]).nL == 8
    for name, (_, ids, longest) in sr.SETTINGS.items():      # the longest track of a batch decides which step kernel runs
        tracks = [n for k in ids for n in list(c[k][0].point_nobs) + list(c[k][0].line_nobs)]
        assert max(tracks) == longest, name
    for k in CASES:
        assert shape(k)[0] <= sr.CAP_POINTS and shape(k)[1] <= sr.CAP_LINES
        assert c[k][1].num_iterations == 1 and c[k][1].marginalization_flag == -1


@pytest.mark.parametrize("case", CASES)
def test_conditions_the_gpu_tests_rely_on(case, oracle_runs, monkeypatch, capfd):
    prob, x0, lin, st = sr.reference(case)
    d2 = prob.opt.huber_delta ** 2
    if len(lin.sq) > 1:       # (case b is one projection factor by definition, case a has none)
        assert (lin.sq > d2).any() and (lin.sq < d2).any(), "one Huber regime only: change the seed of this case"
    assert len(lin.sq) == 0 or np.abs(lin.sq - d2).min() >= 1e-9 * d2, "a residual block sits on the Huber threshold: change the seed"
    wc, rep, log = _oracle(case, oracle_runs, monkeypatch, capfd)
    assert rep.iterations == 1 and rep.num_successful_steps == 1, "the oracle does not accept the first step: change the seed"
    mus = re.findall(r"^it 1 cost .* mu (\S+)$", log, flags=re.M)
    assert len(mus) == 1 and float(mus[0]) == 1e-8, log
    assert st["branch"] == "gauss-newton" and float(st["model_cost_change"]) > 0


@pytest.mark.parametrize("case", CASES)
def test_one_iteration_of_the_oracle_is_x0_plus_the_reference_step(case, oracle_runs, monkeypatch, capfd):
    prob, x0, lin, st = sr.reference(case)
    wc, rep, _ = _oracle(case, oracle_runs, monkeypatch, capfd)
    print("initial_cost error / (eps64 sum |terms|) = %.3g" % (float(abs(sr.LD(rep.initial_cost) - lin.cost)) / lin.unit_cost))
    assert abs(sr.LD(rep.initial_cost) - lin.cost) <= 8 * lin.unit_cost
    delta = np.asarray(st["delta"], np.float64)
    lv = sr.live(lin.H)
    fwd = 8 * EPS * sr.cond2(st["A"][np.ix_(lv, lv)])
    b = {k: fwd * np.linalg.norm(delta[idx]) for k, idx in prob.classes().items()}
    hb = prob.hand_back(prob.plus(x0, delta))
    amax = lambda a: float(np.abs(a).max()) if np.size(a) else 0.0
    lever = max(np.linalg.norm(hb["pose"][i, :3] - hb["pose"][0, :3]) for i in range(sr.NF))
    # after the gauge fix: P_i = R_yaw (p_i - p_0) + P0, R_i = R_yaw r_i, V_i = R_yaw v_i -- the yaw comes from rotation 0
    B_pos = 2 * b["pos"] + 2 * b["rot"] * lever + 8 * EPS * amax(hb["pose"][:, :3])
    B_rot = 2 * b["rot"] + 8 * EPS
    B_sb = b["sb"] + 2 * b["rot"] * amax(hb["sb"][:, :3]) + 8 * EPS * amax(hb["sb"])
    assert amax(hb["pose"][:, :3] - wc.pose[:, :3]) <= B_pos
    assert _qdiff(hb["pose"][:, 3:], wc.pose[:, 3:]) <= B_rot
    assert amax(hb["sb"] - wc.speed_bias) <= B_sb
    assert amax(hb["ex"][:3] - wc.ex_pose[:3]) <= b["ex_pos"] + 8 * EPS * amax(hb["ex"][:3])
    assert _qdiff(hb["ex"][3:], wc.ex_pose[3:]) <= b["ex_rot"] + 8 * EPS
    if not prob.ex_free:
        assert amax(hb["ex"] - wc.ex_pose) <= 8 * EPS
    if prob.nP:
        assert amax(hb["invd"] - wc.inv_depth) <= b["invd"] + 8 * EPS * amax(hb["invd"])
    if prob.nL:
        # a line in its start camera frame: (n, d) = (R^T (n_w - t x d_w), R^T d_w) with |(n_w, d_w)| = 1: an angle error of the
        # line or of the camera rotation turns or rescales it by that angle, a translation error moves n by that length
        plk_o = wc.line_plk[prob.lines]
        reach = 1.0 + max(np.linalg.norm(hb["pose"][i, :3]) for i in range(sr.NF)) + np.linalg.norm(hb["ex"][:3])
        B_plk = reach * (4 * (b["line"] + B_rot + b["ex_rot"]) + 8 * EPS) + 2 * (B_pos + b["ex_pos"])
        assert amax(hb["plk"] - plk_o) <= B_plk
        gone = np.setdiff1d(np.arange(len(wc.line_start)), prob.lines)
        assert np.array_equal(wc.line_plk[gone], prob.w.line_plk[gone])       # untriangulated lines keep the caller's value


def test_the_yardsticks_in_step_ref_are_the_ones_this_machine_measures():
    """the table YARDSTICK is a record of `python tests/step_ref.py`: seeded, so it reproduces up to the libm and the matrix
    product in use.  Held to a factor 4 where the bar depends on it: entries below 1 are floored at 1 by step_ref.bar and are
    rounding noise themselves; they only have to stay below 1."""
    now = sr.measure()
    assert set(now) == set(sr.YARDSTICK) == set(CASES)
    for case, y in now.items():
        for k, val in sr.YARDSTICK[case].items():
            if val < 1.0:
                assert y[k] < 4.0, (case, k, y[k], val)
            else:
                assert 0.25 * val <= y[k] <= 4.0 * val, (case, k, y[k], val)
