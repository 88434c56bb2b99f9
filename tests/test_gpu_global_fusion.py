"""vpl_gf_optimize_batch on the device against the sequential restatement tests/gf_ref.py (the substructured algebra) on the named
chains of tests/gf_inputs.py.

Integers, termination and status are equal.  The solution vector -- the poses, wgps_T_wvio, the final cost -- is held to the
project's bar: max(32 max |x64 - x80|, 1e-12 |x64|_inf), x64 / x80 the restatement's float64 and np.longdouble runs;
tests/test_gf_reference.py holds the two to the same decisions with every deciding quantity 1e-6 away from its threshold.  A chain
solved at S = 4, S = 7 and S >= n agrees within the same bar; a batch follows its items and repeats bit for bit;
vpl_gf_debug_step's g, first step and model cost change are compared with the dense long-double solve of the same system."""
import numpy as np
import pytest

import vplines_slam_amd as v

import gf_inputs
import gf_ref

pytestmark = pytest.mark.gpu

K_BAR = 32
NAMES = list(gf_inputs.CASES)
INTS = ("status", "termination", "iterations", "successful_steps", "unsuccessful_steps")


def chain_input(name):
    g = gf_inputs.case(name)
    return v.GlobalFusionInput(g["local"], g["glob"], g["gps_node"], g["gps_xyz"], g["gps_accuracy"])


def options(name, **changes):
    o = dict(gf_inputs.case(name)["opt"])
    o.update(changes)
    return v.default_gf_options(**o)


def opt_key(name):
    return tuple(sorted(gf_inputs.case(name)["opt"].items()))


def got_dict(res):
    return dict(pose=res.pose, wgps_T_wvio=res.T, final_cost=res.final_cost)


def check(name, res, label=""):
    r64, r80 = gf_inputs.ref_case(name, "f64"), gf_inputs.ref_case(name, "f80")
    print(name, label, {k: getattr(res, k) for k in INTS}, "reference", {k: r64[k] for k in INTS}, r64["verdicts"])
    for k in INTS:
        assert getattr(res, k) == r64[k], (name, k, getattr(res, k), r64[k])
    x64, x80, x = gf_ref.solution(r64), gf_ref.solution(r80), gf_ref.solution(got_dict(res))
    d = float(np.abs(x64 - x80).max())
    bar = max(K_BAR * d, 1e-12 * float(np.abs(x64).max()))
    err = float(np.abs(x - x64).max())
    print("   error %.3g, bar %.3g (|x64 - x80| %.3g), ratio to |x64 - x80| %.3g" % (err, bar, d, err / max(d, 1e-300)))
    assert err <= bar, (name, err, bar, d)
    ic = float(r64["initial_cost"])
    assert abs(res.initial_cost - ic) <= 1e-12 * max(ic, 1e-300) + 32 * abs(ic - float(r80["initial_cost"]))


@pytest.mark.parametrize("name", NAMES)
def test_global_fusion_matches_the_sequential_restatement(gpu_ctx, name):
    res = gpu_ctx.global_fusion([chain_input(name)], options(name))
    check(name, res[0])


@pytest.mark.parametrize("name", ["n9", "n41", "fix_places", "turning", "reject"])
def test_segment_lengths_agree(gpu_ctx, name):
    n = len(gf_inputs.case(name)["local"])
    for S in (4, 7, n, n + 1, 1000):
        res = gpu_ctx.global_fusion([chain_input(name)], options(name, segment=S))
        check(name, res[0], "S = %d" % S)


def test_batch_follows_the_items_and_repeats_bit_for_bit(gpu_ctx):
    plain = [n for n in NAMES if opt_key(n) == (("segment", 4),)]
    assert "ftol" in plain and "no_convergence" in plain and "n1" in plain and "no_fix" in plain   # chains that end early beside a five-iteration one
    first = {}
    for order in (plain, ["no_convergence", "ftol"] + [n for n in plain[::-1] if n not in ("no_convergence", "ftol")], ["ftol", "no_convergence"]):
        inputs = [chain_input(n) for n in order]
        res = gpu_ctx.global_fusion(inputs, v.default_gf_options(segment=4))
        again = gpu_ctx.global_fusion(inputs, v.default_gf_options(segment=4))
        for i, n in enumerate(order):
            check(n, res[i])
            assert res[i].data() == again[i].data(), n
            assert first.setdefault(n, res[i].data()) == res[i].data(), n     # the same bytes in every order and batch
    for group in (["reject"], ["reject", "reject"]):
        res = gpu_ctx.global_fusion([chain_input(n) for n in group], options("reject"))
        for i, n in enumerate(group):
            check(n, res[i])
            assert first.setdefault(n, res[i].data()) == res[i].data(), n


@pytest.mark.parametrize("name", ["n1_fix", "n2", "n4", "n5", "n9", "n41", "fix_places", "single_fix", "all_outside", "outlier", "turning",
                                  "yawed_frame", "default_segment"])
def test_first_step_against_the_dense_long_double_solve(gpu_ctx, name):
    got = gpu_ctx.global_fusion_debug_step(chain_input(name), options(name))
    exact = gf_inputs.ref_case(name, "f80", "dense")["first"]
    own = gf_inputs.ref_case(name, "f64", "chain")["first"]
    ld = np.longdouble
    for key, mine in (("g", got["g"]), ("step", got["step"]), ("model", np.array([got["model_cost_change"]]))):
        ex = np.atleast_1d(np.asarray(exact[key], ld))
        ref_err = float(np.abs(np.atleast_1d(np.asarray(own[key], ld)) - ex).max())
        err = float(np.abs(np.asarray(mine, ld) - ex).max())
        bar = max(K_BAR * ref_err, 1e-12 * float(np.abs(ex).max()))
        print("%s %s: error %.3g, the float64 restatement's %.3g, ratio %.3g, bar %.3g" % (name, key, err, ref_err, err / max(ref_err, 1e-300), bar))
        assert err <= bar, (name, key, err, bar)


def test_wgps_T_wvio_carries_the_last_local_pose_onto_the_last_global_one(gpu_ctx):
    for name in ("n41", "yawed_frame", "n1"):
        g = gf_inputs.case(name)
        res = gpu_ctx.global_fusion([chain_input(name)], options(name))[0]
        T, last, loc = res.T, res.pose[-1], g["local"][-1]
        assert np.array_equal(T[3], [0, 0, 0, 1])
        assert np.abs(T[:3, :3].dot(loc[:3]) + T[:3, 3] - last[:3]).max() <= 1e-12 * max(1.0, np.abs(last[:3]).max())
        Rg, Rl = gf_ref.qmat(last[3:]), gf_ref.qmat(loc[3:])
        assert np.abs(T[:3, :3].dot(Rl) - Rg).max() <= 1e-12
    assert res.iterations == 0 and np.array_equal(res.pose, g["glob"])    # n = 1 without a fix: nothing moves


def test_refusals(gpu_ctx):
    o = v.default_gf_options()
    ref = gf_ref.default_options()
    for f, _ in v.capi.GfOptions._fields_:
        assert getattr(o, f) == ref[f], f
    q = chain_input("n5")
    for bad in (dict(initial_radius=0.0), dict(max_iterations=-1), dict(t_var=0.0), dict(q_var=-1.0), dict(segment=1), dict(segment=-4),
                dict(min_lm_diagonal=0.0), dict(max_consecutive_invalid_steps=0)):
        assert gpu_ctx.global_fusion([q], v.default_gf_options(**bad), check=False) == -1, bad
    ci = q.to_c()
    ci.local = None
    assert gpu_ctx.global_fusion([ci], check=False) == -1
    ci = q.to_c()
    ci.gps_xyz = None
    assert gpu_ctx.global_fusion([ci], check=False) == -1
    ci = q.to_c()
    ci.n = 0
    assert gpu_ctx.global_fusion([ci], check=False) == -1
    g = gf_inputs.case("n5")
    for nodes in ([4, 1], [1, 1], [1, 5], [-1, 4]):
        assert gpu_ctx.global_fusion([v.GlobalFusionInput(g["local"], g["glob"], nodes, g["gps_xyz"], g["gps_accuracy"])], check=False) == -1, nodes
    for acc in ([0.5, 0.0], [-1.0, 0.5], [0.5, np.nan]):
        assert gpu_ctx.global_fusion([v.GlobalFusionInput(g["local"], g["glob"], g["gps_node"], g["gps_xyz"], acc)], check=False) == -1, acc
    n = v.capi.GF_MAX_NODES + 1
    ident = np.tile(np.array([0, 0, 0, 1.0, 0, 0, 0]), (n, 1))
    assert gpu_ctx.global_fusion([v.GlobalFusionInput(ident, ident)], check=False) == -4
    assert gpu_ctx.global_fusion([q] * 65, check=False) == -4            # the fixture's context has max_windows = 64
    # a chain with a non-finite pose fails alone; its neighbour in the batch runs
    broken = g["local"].copy()
    broken[2, 1] = np.nan
    res = gpu_ctx.global_fusion([v.GlobalFusionInput(broken, g["glob"], g["gps_node"], g["gps_xyz"], g["gps_accuracy"]), q], options("n5"))
    assert res[0].termination == v.capi.GF_FAILURE and res[0].iterations == 0 and np.array_equal(res[0].pose, g["glob"])
    assert np.array_equal(res[0].T, np.eye(4))
    check("n5", res[1])
