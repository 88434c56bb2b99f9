"""vpl_select_features_batch / vpl_select_debug_values against the NumPy restatement of FeatureSelector::select
(tests/select_ref.py) on the scenes of tests/select_inputs.py.

Value bar: Omega_kkH, Delta12, f and ub come from select_debug_values with a forced prefix and are compared with the restatement's
long double run; the bar is K max|x64 - x80| over the compared array, never below 1e-12 |x|_inf, K = 32 (the project's bar in
test_gpu_init_relative_pose.py).  Every comparison prints the ratio it meets.
Selection bar: the device's id sequence equals the restatement's; select_inputs.reference asserts, on the CPU and for every scene
it hands out, that the best f stands at least twice the value bar above the second best in every round of both precisions.
The scene "n_imu 1" has no values to compare (the reference's covImu is singular there, tests/test_select_reference.py): it is run
for its counts, its determinism and the guards."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import select_inputs as si
import select_ref as ref
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu

GUARDS = os.environ.get("VPL_DEBUG_GUARDS") == "1"
E_INVALID, E_CAPACITY = -1, -4


def context():
    return v.Context(device=0, max_windows=4, max_points=8, max_point_obs=64, max_lines=8, max_line_obs=64)


def close(ctx):
    if GUARDS:
        assert ctx.debug_guards() == 0
    ctx.close()


def ratio(what, got, x64, x80):
    """max |got - x80| over the bar of the compared array; NaN must stand where the restatement has NaN"""
    got, x64, x80 = (np.asarray(a, dtype=np.longdouble) for a in (got, x64, x80))
    assert np.array_equal(np.isnan(got), np.isnan(x80)), what
    ok = ~np.isnan(x80)
    if not ok.any():
        return 0.0
    bar = si.value_bar(x64, x80)
    err = float(np.abs(got[ok] - x80[ok]).max())
    r = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    print("%-42s err %.3g bar %.3g ratio %.3g" % (what, err, bar, r))
    return r


@functools.lru_cache(maxsize=None)
def one_round(name, prefix):
    """the restatement's values of one round after the forced prefix, in the two precisions"""
    par, s = si.scene(name)
    return tuple(ref.run(dt, par, s, prefix=prefix, kappa=1) for dt in (np.float64, np.longdouble))


def check_values(ctx, name, prefix=()):
    par, s = si.scene(name)
    r64, r80 = one_round(name, tuple(prefix))
    dev = ctx.select_debug_values(par, s, prefix)
    assert ratio(name + ": Omega_kkH", dev["omega"], r64["omega"], r80["omega"]) <= 1.0
    n_new = len(s.new_id)
    assert ratio(name + ": Delta12 new", dev["delta12"][:n_new], r64["d12_new"], r80["d12_new"]) <= 1.0
    if len(s.used_x):
        assert ratio(name + ": Delta12 used", dev["delta12"][n_new:], r64["d12_used"], r80["d12_used"]) <= 1.0
    full = lambda r, k: np.array([dict(zip(r["rounds"][0][0], r["rounds"][0][k])).get(int(i), np.nan) if r["rounds"] else np.nan for i in s.new_id],
                                 dtype=np.longdouble)
    assert ratio(name + ": f", dev["f"], full(r64, 2), full(r80, 2)) <= 1.0
    assert ratio(name + ": ub", dev["ub"], full(r64, 1), full(r80, 1)) <= 1.0
    return dev


def check_selection(ctx, name):
    r = si.reference(name)
    par, s, r64, r80 = r["par"], r["scene"], r["r64"], r["r80"]
    out = ctx.select_features(par, [s])[0]
    assert list(out["ids"]) == r80["ids"], (name, list(out["ids"]), r80["ids"])
    assert out["n_invisible"] == len(r80["invisible"]) and out["n_candidates"] == len(s.new_id) - len(r80["invisible"])
    assert out["n_ineligible"] == 0
    for k in range(len(out["ids"])):
        assert abs(out["f"][k] - float(r80["f"][k])) <= r["bar_f"][k], (name, k)
    return out


# ---- the scenes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1 candidate", "12 candidates", "63 candidates", "64 candidates", "65 candidates", "kappa 1", "kappa above",
                                  "empty cloud", "cloud of 1", "no used", "n_imu 2", "own horizon", "behind"])
def test_values_and_selection(name):
    ctx = context()
    check_values(ctx, name)
    r = si.reference(name)
    if len(r["r80"]["ids"]) > 1:
        check_values(ctx, name, tuple(r["r80"]["ids"][:-1]))      # the last round the restatement plays, its prefix forced
    check_selection(ctx, name)
    close(ctx)


def test_two_identical_candidates_the_higher_id_first_then_the_lower():
    ctx = context()
    dev = check_values(ctx, "2 identical")
    assert dev["ub"][0] == dev["ub"][1] and dev["f"][0] == dev["f"][1]        # the same bits: the collapse is exact
    out = check_selection(ctx, "2 identical")
    assert list(out["ids"]) == [1001, 1000]
    close(ctx)


def test_one_past_the_greedy_work_group():
    ctx = context()
    name = "past the work-group"
    assert len(si.scene(name)[1].new_id) == si.GREEDY_THREADS + 1
    check_values(ctx, name)
    check_values(ctx, name, tuple(si.reference(name)["r80"]["ids"][:2]))
    check_selection(ctx, name)
    close(ctx)


def test_larger_shape_through_a_forced_prefix():
    """200 candidates: value by value after a prefix of five, not through the full greedy (its gaps fall below the arithmetic)"""
    ctx = context()
    par, s = si.scene("bench 200")
    first = tuple(int(i) for i in s.new_id[[3, 77, 150, 199, 42]])
    check_values(ctx, "bench 200", first)
    close(ctx)


def test_kappa_zero_selects_nothing():
    ctx = context()
    out = check_selection(ctx, "kappa 0")
    assert len(out["ids"]) == 0 and out["n_candidates"] == 12
    close(ctx)


def test_a_feature_behind_a_future_camera_still_counts():
    """the scene "behind" has candidates that a future frame sees at z < 0 (asserted on the CPU by select_inputs.reference); the
    device gives them a Delta12 like the restatement's (test_values_and_selection) and may select them"""
    ctx = context()
    r = si.reference("behind")
    behind = si.behind_and_visible(r["par"], r["scene"], r["r64"])
    dev = ctx.select_debug_values(r["par"], r["scene"])
    for i in behind:
        k = list(r["scene"].new_id).index(i)
        assert dev["delta12"][k].any() and np.isfinite(dev["f"][k])
    assert set(behind) & set(ctx.select_features(r["par"], [r["scene"]])[0]["ids"])
    close(ctx)


def test_a_candidate_no_future_frame_sees():
    ctx = context()
    dev = check_values(ctx, "invisible")
    assert np.isnan(dev["f"][1]) and np.isnan(dev["ub"][1]) and not dev["delta12"][1].any()
    out = check_selection(ctx, "invisible")
    assert out["n_invisible"] == 1 and 1001 not in out["ids"]
    close(ctx)


def test_huge_variances_every_logdet_below_minus_one_nothing_selected():
    ctx = context()
    dev = check_values(ctx, "huge variances")
    assert np.nanmax(dev["f"]) < -1.0
    out = check_selection(ctx, "huge variances")
    assert len(out["ids"]) == 0
    close(ctx)


def test_one_imu_sample_runs_and_repeats():
    """the reference's covImu is singular for n_imu = 1: nothing to compare, but the call ends, stays inside its arrays (guards),
    gives the same bits twice, and whatever the rounding noise over the zero determinant yields obeys the rules of the greedy
    loop: what is selected is distinct, a candidate, and has a finite f > -1; and when fewer than min(kappa, candidates) are
    selected, the round that ended the loop evaluated every candidate that was left, so a call that selects nothing with no
    finite value anywhere counts every candidate as ineligible once"""
    ctx = context()
    par, s = si.scene("n_imu 1")
    a, b = ctx.select_features(par, [s])[0], ctx.select_features(par, [s])[0]
    print("n_imu 1: selected %s f %s ineligible %d candidates %d" % (list(a["ids"]), list(a["f"]), a["n_ineligible"], a["n_candidates"]))
    assert len(a["ids"]) <= s.kappa and a["n_candidates"] + a["n_invisible"] == len(s.new_id)
    assert a["ids"].tobytes() == b["ids"].tobytes() and a["f"].tobytes() == b["f"].tobytes()
    k = len(a["ids"])
    assert len(set(a["ids"])) == k and set(a["ids"]) <= set(s.new_id) and np.isfinite(a["f"]).all() and (a["f"] > -1.0).all()
    dev = ctx.select_debug_values(par, s)
    if not np.isfinite(dev["omega"]).all():           # the inverse overflowed: no pivot can be good
        assert k == 0 and a["n_ineligible"] == a["n_candidates"] and np.isnan(dev["f"]).all()
    close(ctx)


def test_batch_of_two_sizes_equals_the_solo_runs_bit_for_bit_and_repeats():
    ctx = context()
    par = si.params()
    a, b = si.scene("12 candidates")[1], si.scene("65 candidates")[1]
    both = ctx.select_features(par, [a, b])
    again = ctx.select_features(par, [a, b])
    solo = [ctx.select_features(par, [a])[0], ctx.select_features(par, [b])[0]]
    swapped = ctx.select_features(par, [b, a])
    for k in range(2):
        assert len(both[k]["ids"]) > 0
        for other in (again[k], solo[k], swapped[1 - k]):
            assert both[k]["ids"].tobytes() == other["ids"].tobytes() and both[k]["f"].tobytes() == other["f"].tobytes()
            assert both[k]["n_invisible"] == other["n_invisible"] and both[k]["n_ineligible"] == other["n_ineligible"]
    d1, d2 = ctx.select_debug_values(par, b, (1015,)), ctx.select_debug_values(par, b, (1015,))
    assert all(d1[k].tobytes() == d2[k].tobytes() for k in d1)
    close(ctx)


def test_launches_do_not_depend_on_kappa():
    ctx = context()
    par, s = si.scene("65 candidates")
    stats = []
    for kappa in (1, 40):
        out = ctx.select_features(par, [v.SelectInput.of(s, kappa=kappa)])[0]
        assert len(out["ids"]) == kappa
        stats.append(ctx.select_stats())
    assert stats[0][0] == stats[1][0] == 3 and stats[0][1:] == stats[1][1:]
    close(ctx)


def test_refusals():
    ctx = context()
    par, s = si.scene("12 candidates")
    sel = lambda **kw: ctx.select_features(par, [v.SelectInput.of(s, **kw)], check=False)
    assert sel(n_imu=0) == E_INVALID and sel(delta_imu=0.0) == E_INVALID and sel(delta_imu=float("nan")) == E_INVALID and sel(kappa=-1) == E_INVALID
    n = v.capi.SEL_MAX_FEATURES + 1
    assert sel(new_id=np.arange(n), new_x=np.zeros(n), new_y=np.zeros(n), new_prob=np.ones(n)) == E_CAPACITY
    assert sel(used_x=np.zeros(n), used_y=np.zeros(n)) == E_CAPACITY and sel(cloud=np.ones((n, 3))) == E_CAPACITY
    keep = v.SelectInput.of(s)
    for member in ("new_id", "new_x", "new_prob", "used_y", "cloud"):
        ci = keep.to_c()
        setattr(ci, member, None)
        assert ctx.select_features(par, [ci], check=False) == E_INVALID, member
    assert ctx.select_features(par, [s] * 5, check=False) == E_CAPACITY            # max_windows = 4
    assert sel(new_id=np.r_[s.new_id[:-1], s.new_id[0]]) == E_INVALID                # an id twice
    assert ctx.select_debug_values(par, v.SelectInput.of(s, n_imu=0), check=False) == E_INVALID
    assert len(ctx.select_features(par, [s])[0]["ids"]) == 6                        # the context is still good
    close(ctx)


def test_everything_under_debug_guards_in_a_fresh_process():
    """every test above once more with VPL_DEBUG_GUARDS=1 (read when a context is made): the pattern behind every device array the
    call takes is checked inside the call, the context's own when it is closed"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VPL_DEBUG_GUARDS="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    code = ("import test_gpu_select as t; assert t.GUARDS\n"
            "for name in sorted(dir(t)):\n"
            "    if name.startswith('test_') and 'fresh_process' not in name:\n"
            "        f = getattr(t, name)\n"
            "        for m in getattr(f, 'pytestmark', []):\n"
            "            if m.name == 'parametrize':\n"
            "                [f(a) for a in m.args[1]]\n"
            "                break\n"
            "        else:\n"
            "            f()\n"
            "print('guards ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "guards ok" in r.stdout
