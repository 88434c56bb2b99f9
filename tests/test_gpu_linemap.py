"""The line-map stage on the device against linemap_ref.py's long-double values (checked on the CPU by test_linemap_reference.py):
k_triangulate and k_triangulate_points through Context.triangulate_lines / triangulate_points, k_line_opt in its three lane
layouts and k_gauge's setLineOrth + removeLineOutlier through Context.only_line_opt, the loop stopped after k = 1, 2, ... iterations
and compared with the reference's state after k iterations.

Exact: the report's iterations, successful steps and termination, the erase flags and their count, the triangulation flags, the
bits of everything a call must not touch.  In units (rho = error / unit; nothing is tuned to the device or the oracle): costs in
eps64 x cost, lines after the loop as normalised Pluecker vectors up to the common sign in eps64 per entry, triangulated vectors and
inverse depths in eps64 |value| + what rounding each input alone does to them.  Bar = 8 x max(what linemap_ref's own float64 run
reaches on the case -- for onlyLineOpt at that k --, 1) (linemap_ref.YARDSTICK).  A device result that takes another decision than
the reference fails: every decision of every case has a margin of 1e3 x the float64 runs' deviation, asserted on the CPU."""
import numpy as np
import pytest

import linemap_ref as lr
import vplines_slam_amd as v

pytestmark = pytest.mark.gpu
_failed = {}
SWEPT = ["lo_generic", "lo_reject", "lo_reject2", "lo_four", "lo_three"] + list(lr.OUT_RULE)


def _guard(f, *a, **kw):
    """after a failed device call nothing more of this file is sent to the device"""
    if _failed:
        raise _failed["first"]
    try:
        return f(*a, **kw)
    except BaseException as e:
        _failed["first"] = e
        raise


def _with_context(f, max_windows=1, max_points=4, max_lines=12, line_obs=11):
    def run():
        ctx = v.Context(device=0, max_windows=max_windows, max_points=max_points, max_point_obs=max_points * 11, max_lines=max_lines,
                        max_line_obs=max_lines * line_obs)
        try:
            return f(ctx)
        finally:
            ctx.close()
    return _guard(run)


def _sweep_on_device(name, max_lines, line_obs=11):
    """[(k, report, window)] of the case under num_iterations = k for every k of its sweep, in a context of max_lines lines"""
    w = lr.lo_cases()[name][0]

    def run(ctx):
        out = []
        for k in lr.sweep(name):
            w2 = w.copy()
            out.append((k, ctx.only_line_opt([w2], lr.options(k))[0], w2))
        return out
    return _with_context(run, max_lines=max_lines, line_obs=line_obs)


def _hold(name, runs, layout):
    late = []
    for k, rep, w2 in runs:
        got = lr.lo_check(name, k, rep, w2)
        y = lr.YARDSTICK[name]
        j = lr.sweep(name).index(k)
        for what, val in got.items():
            b = lr.lo_bar(name, what, None if what == "cost0" else k)
            print("%s k_line_opt<%d> k = %d %s rho %.3g (bar %.3g; float64 restatement %.3g)"
                  % (name, layout, k, what, val, b, y[what] if what == "cost0" else y[what][j]))
            if not val <= b:
                late.append((name, layout, k, what, val, b))
    assert not late, late


@pytest.mark.parametrize("max_lines", list(lr.LANES))
@pytest.mark.parametrize("name", SWEPT)
def test_only_line_opt_after_every_iteration_in_every_lane_layout(name, max_lines):
    """4, 2 and 1 lanes per line (contexts of 12, 100 and 200 lines): the 4 x 4 solve per line, the accept / reject decision on the
    block-summed cost, the radius schedule with the kept diagonal, the candidate evaluation, the tolerances and the iteration cap,
    then setLineOrth and the three erase rules"""
    assert lr.LANES[max_lines] == (4 if 4 * max_lines <= 256 else 2 if 2 * max_lines <= 256 else 1)
    _hold(name, _sweep_on_device(name, max_lines), lr.LANES[max_lines])


@pytest.mark.parametrize("name", list(lr.FULL))
def test_only_line_opt_with_every_lane_live(name):
    """max_lines = the number of triangulated lines = 64, 128, 256: all 256 lanes live in the three layouts; 65: the first size
    with two lanes per line, the last wave partly live"""
    n = lr.FULL[name]
    layout = 4 if 4 * n <= 256 else 2 if 2 * n <= 256 else 1
    assert layout * n == 256 or n == 65
    _hold(name, _sweep_on_device(name, n, line_obs=3), layout)


# ---- triangulateLine -------------------------------------------------------------------------------------------------------------
def _hold_tl(name, w2):
    got = lr.tl_check(name, w2)
    print("%s plk rho %.3g (bar %.3g; float64 restatement %.3g)" % (name, got["plk"], lr.bar(name, "plk"), lr.YARDSTICK[name]["plk"]))
    assert got["plk"] <= lr.bar(name, "plk"), (name, got)


@pytest.mark.parametrize("name", ["tl_generic", "tl_threshold", "tl_one_obs", "tl_keep", "tl_stride"])
def test_triangulate_lines(name):
    """flags exact, vectors in units, untouched lines bit-equal; tl_stride: 129 lines for the 128 threads of k_triangulate"""
    w2 = lr.tl_cases()[name].copy()
    n = len(w2.line_start)
    _with_context(lambda ctx: ctx.triangulate_lines([w2]), max_lines=max(n, 12), line_obs=11 if n < 20 else 3)
    _hold_tl(name, w2)


def test_triangulate_lines_of_three_windows_in_one_call():
    """windows of 5, 1 and 9 lines: the per-window offsets"""
    names = ["tl_batch%d" % i for i in range(3)]
    ws = [lr.tl_cases()[n].copy() for n in names]
    _with_context(lambda ctx: ctx.triangulate_lines(ws), max_windows=3)
    for n, w2 in zip(names, ws):
        _hold_tl(n, w2)


# ---- triangulate (points) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lr.tp_cases()))
def test_triangulate_points(name):
    """inverse depths in units (tp_stride: 16 tracks in units, the rest in eps64 |value| against the case's yardstick), init_depth's
    exact bits where the depth is below 0.1, tracks that have a depth (-0.0 included) bit-equal"""
    w2 = lr.tp_cases()[name].copy()
    _with_context(lambda ctx: ctx.triangulate_points([w2], lr.INIT_DEPTH), max_points=max(len(w2.point_start), 4), max_lines=4)
    got = lr.tp_check(name, w2)
    for what, val in got.items():
        print("%s %s rho %.3g (bar %.3g; float64 restatement %.3g)" % (name, what, val, lr.bar(name, what), lr.YARDSTICK[name][what]))
        assert val <= lr.bar(name, what), (name, what, val)
