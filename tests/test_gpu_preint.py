"""vpl_preintegrate_batch (k_preintegrate, the lane-spread preint_steps of ba_factors.h) against the long-double restatement of
integration_base.h (preint_ref.py), in its units, bar 32 -- the bar test_preint_reference.py earns on the CPU, where the float64
restatement, the oracle and preint_step all stay below 8 units on the same cases.  Nothing here is measured on the kernel.

* every case and every batch of preint_inputs.py: the deltas, every block of J and P, structural zeros exact, sum_dt, the
  asymmetry of P, linearized_ba / linearized_bg bit for bit;
* position independence, bit for bit: an interval's result depends neither on its group in the block, nor on n, nor on its
  neighbours' lengths (which set the block's step count), nor on where its samples lie;
* an empty interval whose offset points at a row of NaN that belongs to nobody is the identity, and its neighbours are untouched;
* negative offset / nsamples are refused with VPL_E_INVALID and the context goes on working.

Measured on the MI355X (units; bar 32): worst 1.2 (P of the one-sample interval), per quantity dp 0.42, dq 0.24, dv 0.11, J 0.76,
P 1.2, asymmetry of P 0.34; per case in DESIGN.md, "IMU pre-integration against long double"."""
import ctypes as C

import numpy as np
import pytest

import preint_inputs as pi
import preint_ref as pr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
VPL_E_INVALID = -1
FIELDS = ("sum_dt", "delta_p", "delta_q", "delta_v", "jacobian", "covariance", "linearized_ba", "linearized_bg")


def _bits(p):
    return np.concatenate([np.atleast_1d(np.array(getattr(p, f), np.float64)).ravel() for f in FIELDS])


def _same_bits(a, b):
    return np.array_equal(_bits(a).view(np.uint64), _bits(b).view(np.uint64))


def _run(ctx, arr, noise=pi.NOISE):
    return ctx.preintegrate(*arr, pr.options(noise))


def _hold(out, name):
    """one interval of a device result against the long-double run of its case -> the errors in units"""
    c, ref = pi.cases()[name], pr.reference(name)
    o = pr.Out(out)
    assert np.array_equal(o.lba, c["ba"]) and np.array_equal(o.lbg, c["bg"]), "linearized_ba / linearized_bg are copies"
    e = pr.errors(o, ref)                      # asserts the structural zeros and sum_dt
    assert pr.worst(e) <= pr.BAR and e["asym"] <= pr.BAR, (name, e)
    return e


@pytest.mark.parametrize("batch", list(pi.batches()))
def test_batch_against_long_double(gpu_ctx, batch):
    names, arr = pi.batches()[batch]
    pre = _run(gpu_ctx, arr, pi.cases()[names[0]]["noise"])
    for k, name in enumerate(names):
        e = _hold(pre[k], name)
        print("%-10s %-15s dp %.3g dq %.3g dv %.3g J %.3g P %.3g asym %.3g units" % (batch, name, e["dp"], e["dq"], e["dv"], e["J"], e["P"], e["asym"]))


def test_the_batches_cover_what_they_claim():
    b = pi.batches()
    assert sorted(len(names) for names, _ in b.values()) == [1, 1, 4, 5, 7, 15, 15]
    assert list(b["block_0_1_37_3"][1][1]) == [0, 1, 37, 3]
    assert set(b["all"][0]) | {"default20"} == set(pi.COUNTS)
    off, ns = b["scattered"][1][0], b["scattered"][1][1]
    assert np.any(np.diff(off[ns > 0]) < 0), "offsets not monotone"
    for names, arr in b.values():               # no interval, empty or not, points outside the rows handed in
        assert np.all(arr[0] + np.maximum(arr[1], 1) <= len(arr[2]))


def test_position_independence_bit_for_bit(gpu_ctx):
    ref = None
    for names, arr, k in pi.position_batches():
        assert names[k] == pi.SUBJECT
        out = _run(gpu_ctx, arr)[k]
        ref = out if ref is None else ref
        assert _same_bits(out, ref), (names, k)
    _hold(ref, pi.SUBJECT)
    groups = sorted({k % 4 for n, _, k in pi.position_batches() if len(n) == 4})
    assert groups == [0, 1, 2, 3] and {len(n) for n, _, _ in pi.position_batches()} == {1, 4, 5, 7}
    # and the intervals of `scattered` are those of `all`, wherever their samples lie
    b = pi.batches()
    a, s = _run(gpu_ctx, b["all"][1]), _run(gpu_ctx, b["scattered"][1])
    for k, name in enumerate(b["all"][0]):
        assert _same_bits(a[k], s[k]), name


def test_empty_interval_beside_a_row_of_nan(gpu_ctx):
    """an empty interval runs the block's nmax steps at dt = 0 like any group past its own count; it must not read a sample row
    (0 * NaN is NaN) and returns the identity, whatever lies at its offset"""
    names, arr, k = pi.nan_row_batch()
    pre = _run(gpu_ctx, arr)
    o = pr.Out(pre[k])
    assert o.sum_dt == 0.0 and not o.dp.any() and not o.dv.any() and np.array_equal(o.q, [0, 0, 0, 1])
    assert np.array_equal(o.J, np.eye(15)) and np.array_equal(o.P, np.zeros((15, 15)))
    _hold(pre[k], "n0")
    alone = {name: _run(gpu_ctx, pi.assemble([name], fill=0.5))[0] for name in names if name != "n0"}
    for i, name in enumerate(names):
        if i != k:
            assert _same_bits(pre[i], alone[name]), name
            _hold(pre[i], name)


def test_negative_offset_and_count_are_refused(gpu_ctx):
    names = ["n3", "n20", "n1"]
    arr = pi.assemble(names, fill=0.5)
    good = _run(gpu_ctx, arr)
    for which, idx in ((0, 1), (1, 0), (1, 2)):
        bad = [a.copy() for a in arr]
        bad[which][idx] = -1
        out = (v.Preintegration * len(names))()
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        opt = pr.options(pi.NOISE)
        rc = gpu_ctx.lib.vpl_preintegrate_batch(gpu_ctx.h, len(names), bad[0].ctypes.data_as(ip), bad[1].ctypes.data_as(ip),
                                                *(a.ctypes.data_as(dp) for a in bad[2:]), C.byref(opt), out)
        assert rc == VPL_E_INVALID, (which, idx, rc)
    again = _run(gpu_ctx, arr)                 # the context still works, and gives the same bits
    for k in range(len(names)):
        assert _same_bits(good[k], again[k])
        _hold(again[k], names[k])
