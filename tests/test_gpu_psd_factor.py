"""The pivoted Cholesky factor that turns k_marg's kept block into the next prior (csrc/ba_psd.h), every hand-written form of
it -- psd_pivoted_cholesky_wave<16>, _wave<48> (on 256 and on 512 threads), _wave4<19, 4> and the work-group version -- on
crafted matrices through vpl_ba_debug_psd_factor (k_psd_factor: k_marg's geometry and k_marg's own write-out, one work-group
per case, one launch per form), and the same checks on the kept blocks of real windows through k_marg itself.

The reference is the rule restated in long double (tests/psd_factor_ref.py; tests/test_psd_factor_reference.py shows that it
stays inside the bars on its own).  Every bar is derived (psd_factor_ref.check_factor); none is taken from the device.

Last: batches whose windows keep different sizes.  Every work-group of k_marg lays its LDS out for its own kept size and the
dispatch is sized for the largest layout of any size up to the batch's (csrc/ba_marg_layout.h, marg_lds_doubles): a window
gives in such a batch what it gives alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import psd_factor_ref as R
import vplines_slam_amd as v
from vplines_slam_amd import capi

pytestmark = pytest.mark.gpu

FORMS = {
    "wave16@256": (capi.PSD_WAVE16, 256, R.N_WAVE16),
    "wave48@256": (capi.PSD_WAVE48, 256, R.N_WAVE48),
    "wave48@512": (capi.PSD_WAVE48, 512, R.N_WAVE48),
    "wave4@512": (capi.PSD_WAVE4, 512, R.N_WAVE4),
    "workgroup@256": (capi.PSD_WORKGROUP, 256, R.N_WORKGROUP),
    "workgroup@512": (capi.PSD_WORKGROUP, 512, R.N_WORKGROUP),
}


class World:
    def __init__(self):
        self.cases = R.cases_for(R.N_WORKGROUP)
        self.refs = [R.pivoted_cholesky(c.A, c.b, c.abs_tol, c.rel_tol) for c in self.cases]
        self.ctx = v.Context(device=0, max_windows=1, max_points=8, max_point_obs=88, max_lines=8, max_line_obs=88)
        self.out = {}

    def pick(self, key):
        sizes = FORMS[key][2]
        return [i for i, c in enumerate(self.cases) if c.n in sizes]

    def launch(self, key):
        form, threads, _ = FORMS[key]
        idx = self.pick(key)
        res = self.ctx.debug_psd_factor(form, threads, [(self.cases[i].A, self.cases[i].b, self.cases[i].abs_tol, self.cases[i].rel_tol)
                                                        for i in idx])
        assert not isinstance(res, int), (key, res)
        return dict(zip(idx, res))

    def run(self, key):
        if key not in self.out:
            self.out[key] = self.launch(key)
        return self.out[key]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


def test_case_list_meets_the_input_condition(world):
    for c, ref in zip(world.cases, world.refs):
        R.check_input_condition(c, ref)
    for key in FORMS:
        for n in FORMS[key][2]:
            ranks = {world.refs[i].rank for i in world.pick(key) if world.cases[i].n == n}
            assert ranks >= {0, 1, n // 2, n - 1, n}, (key, n, ranks)


@pytest.mark.parametrize("key", list(FORMS))
def test_form_gives_the_references_factor(world, key):
    """rank, perm (tail included), the factor bound, the structure and the r0 bound, per case"""
    res = world.run(key)
    worst = [0.0, 0.0]
    for i, (rank, perm, J0, r0) in res.items():
        c, ref = world.cases[i], world.refs[i]
        assert rank != -1, (key, c.name, "wave4 gave up a wait")
        q = R.check_factor(c.A, c.b, rank, perm, J0, r0, ref.rank, ref.rank, ref.S, ref.perm, (key, c.name))
        worst = [max(a, b) for a, b in zip(worst, q)]
    print("%s: %d cases, at most %.3f of the factor bar and %.3f of the r0 bar" % (key, len(res), worst[0], worst[1]))


def _same_bits(world, ka, kb):
    a, b = world.run(ka), world.run(kb)
    common = sorted(set(a) & set(b))
    assert common
    diff = []
    for i in common:
        (ra, pa, Ja, ya), (rb, pb, Jb, yb) = a[i], b[i]
        assert ra == rb and np.array_equal(pa, pb), (ka, kb, world.cases[i].name)
        nd = int((Ja.view(np.uint64) != Jb.view(np.uint64)).sum() + (ya.view(np.uint64) != yb.view(np.uint64)).sum())
        if nd:
            diff.append((world.cases[i].name, nd, float(np.nanmax(np.abs(Ja - Jb)))))
    assert not diff, (ka, kb, "entries that differ (case, count, max)", diff[:8], len(diff))
    return len(common)


def test_forms_give_the_same_bits(world):
    """the claim of the comments in csrc/ba_psd.h: the one-wave forms, on either thread count, and the work-group version do
    the same arithmetic per entry"""
    n = [_same_bits(world, "wave48@256", "wave48@512"), _same_bits(world, "wave16@256", "wave48@256"),
         _same_bits(world, "workgroup@256", "workgroup@512"), _same_bits(world, "wave48@256", "workgroup@256"),
         _same_bits(world, "wave16@256", "workgroup@512")]
    print("bit-identical J0 and r0 over %s common cases" % n)


def test_wave4_agrees_in_rank_and_perm_and_repeats_itself(world):
    """wave4 rounds 1 / sqrt(pivot) differently (its comment says so): same rank and perm as the other forms, the same bars
    (test_form_gives_the_references_factor), and the same bits from launch to launch"""
    a, wg = world.run("wave4@512"), world.run("workgroup@512")
    for i in a:
        assert a[i][0] == wg[i][0] and np.array_equal(a[i][1], wg[i][1]), world.cases[i].name
    b = world.launch("wave4@512")
    for i in a:
        assert a[i][0] == b[i][0] and np.array_equal(a[i][1], b[i][1]), world.cases[i].name
        assert a[i][2].tobytes() == b[i][2].tobytes() and a[i][3].tobytes() == b[i][3].tobytes(), world.cases[i].name


def test_other_pairings_are_refused_without_a_launch(world):
    one = lambda n: [(np.eye(n), np.ones(n), 1e-8, 0.0)]
    for form, threads, n in ((capi.PSD_WAVE16, 512, 8), (capi.PSD_WAVE4, 256, 60), (capi.PSD_WAVE48, 128, 8), (capi.PSD_WORKGROUP, 1024, 8),
                             (capi.PSD_WORKGROUP, 64, 8), (4, 256, 8), (-1, 256, 8), (capi.PSD_WAVE16, 256, 17), (capi.PSD_WAVE48, 256, 49),
                             (capi.PSD_WAVE48, 512, 49), (capi.PSD_WAVE4, 512, 77), (capi.PSD_WORKGROUP, 256, 81)):
        assert world.ctx.debug_psd_factor(form, threads, one(n)) == -1, (form, threads, n)
    # ... also when only one case of the batch is out of range
    assert world.ctx.debug_psd_factor(capi.PSD_WAVE16, 256, one(8) + one(17)) == -1
    assert world.ctx.debug_psd_factor(capi.PSD_WAVE16, 256, []) == -1
    res = world.ctx.debug_psd_factor(capi.PSD_WAVE16, 256, one(16))
    assert res[0][0] == 16 and np.array_equal(res[0][2], np.eye(16))


# ---- the same checks through k_marg itself ------------------------------------------------------------------------------
KMARG_ABS, KMARG_REL = 1e-8, 0.0     # kMargEps, kMargNoiseRel


def _kept_block_raw(ctx, w):
    A = np.zeros(80 * 80)
    b = np.zeros(80)
    dp = C.POINTER(C.c_double)
    n = ctx.lib.vpl_ba_debug_marg_Ab(ctx.h, w, A.ctypes.data_as(dp), b.ctypes.data_as(dp))
    assert n > 0
    return A[: n * n].reshape(n, n).copy(), b[:n].copy()


def _kept_block(ctx, w):
    A, b = _kept_block_raw(ctx, w)
    return 0.5 * (A + A.T), b       # as marg_body symmetrises the copy it factors


def _check_pivoted_factor(A, b, J0, r0, tag):
    """k_marg's J0, r0 against its own kept block.  Windows do not keep their pivots a factor 10 away from tol: the rank may
    lie anywhere between the reference's pivots above 10 tol and those above tol / 10, and the factor bound takes the largest
    trailing block over that range.  k_marg does not hand perm out; it is read off J0 (below) and then has to pass the
    structure checks like a perm the kernel returned."""
    n = A.shape[0]
    lo, hi, S, ref = R.rank_window(A, b, KMARG_ABS, KMARG_REL)
    assert not np.isnan(J0).any() and not np.isnan(r0).any(), tag
    rank = int((np.abs(J0).max(axis=1) > 0).sum())
    # row k's pivot column is zero in every later row and not taken yet.  Where several columns are (a never-pivoted index
    # whose row of A is a multiple of the pivot's has |l_tk| = l_kk and nothing below either), the reference's pivot of that
    # step if it is among them, else the largest entry of the row (|l_tk| <= l_kk under diagonal pivoting)
    perm, free = [], list(range(n))
    for k in range(rank):
        later_zero = [j for j in free if np.all(J0[k + 1:, j] == 0.0)]
        assert later_zero, (tag, "row %d has no pivot column" % k)
        want = int(ref.perm[k]) if k < ref.rank else -1
        j = want if want in later_zero else max(later_zero, key=lambda j: abs(J0[k, j]))
        perm.append(j)
        free.remove(j)
    perm += free
    q = R.check_factor(A, b, rank, perm, J0, r0, lo, hi, S, None, tag)
    return rank, lo, hi, q


def _check_all(ctx, pri, nW, tag, want_n=None):
    out = []
    for i in range(nW):
        A, b = _kept_block(ctx, i)
        assert pri[i].n == A.shape[0] and (want_n is None or A.shape[0] == want_n), (tag, i, pri[i].n, A.shape[0])
        out.append(_check_pivoted_factor(A, b, pri[i].J().copy(), pri[i].r().copy(), (tag, i)))
    return out


def _report(tag, rows):
    print("%s: ranks %s (allowed %s), at most %.3f of the factor bar, %.3f of the r0 bar" % (
        tag, [r[0] for r in rows], [(r[1], r[2]) for r in rows], max(r[3][0] for r in rows), max(r[3][1] for r in rows)))


def _set_big(monkeypatch, big):
    if big:
        monkeypatch.setenv("VPL_BA_MARG_BIG", "1")
    else:
        monkeypatch.delenv("VPL_BA_MARG_BIG", raising=False)


def _bench_ctx(nw, cfg, pobs):
    return v.Context(device=0, max_windows=nw, max_points=cfg.n_points, max_point_obs=pobs, max_lines=cfg.n_lines,
                     max_line_obs=cfg.n_lines * 11)


@pytest.mark.parametrize("big", [0, 1])
def test_k_marg_on_the_benchmark_windows(monkeypatch, big):
    """n = 45 under MARGIN_OLD (k_marg<256>, or <512> with VPL_BA_MARG_BIG=1); under MARGIN_SECOND_NEW behind priors that hold
    pose 9 (windows with tracks over all 11 frames in front: a benchmark prior holds poses 0..4 only and passes through)"""
    _set_big(monkeypatch, big)
    opt = v.default_options()
    cfg = v.workload.config(200, 80)
    ctx = _bench_ctx(8, cfg, cfg.n_points * 11)
    B, keep = v.workload.primed_batch(ctx, list(range(8)), cfg, opt)
    _report("MARGIN_OLD, A windows", _check_all(ctx, keep, 8, "A", 45))
    pri, rep = ctx.solve_windows(B, opt)
    _report("MARGIN_OLD, B windows", _check_all(ctx, pri, 8, "B", 45))
    cfgA = v.workload.config(200, 80)
    cfgA.track_len = 11
    A2 = [v.workload.generate(v.workload.seed_for(3, 600 + i), cfgA, 0.4 * i) for i in range(8)]
    B2 = [v.workload.generate(v.workload.seed_for(3, 700 + i), cfg, 0.4 * i + cfg.kf_dt) for i in range(8)]
    v.workload.set_preintegrations(A2 + B2, ctx.preintegrate(*v.workload.imu_batch_arrays(A2 + B2), opt))
    p1, _ = ctx.solve_windows(A2, opt)
    _report("MARGIN_OLD, 11-frame tracks", _check_all(ctx, p1, 8, "A2"))
    keep2 = (capi.Prior * 8)()
    C.memmove(keep2, p1, C.sizeof(keep2))
    for i in range(8):
        B2[i].prior = keep2[i]
    opt.marginalization_flag = v.capi.MARGIN_SECOND_NEW
    p2, rep = ctx.solve_windows(B2, opt)
    assert all(rep[i].prior_m == 6 and p2[i].n == keep2[i].n - 6 for i in range(8))
    _report("MARGIN_SECOND_NEW", _check_all(ctx, p2, 8, "SECOND_NEW"))
    ctx.close()


@pytest.mark.parametrize("big", [0, 1])
def test_k_marg_on_the_steady_state(monkeypatch, big):
    _set_big(monkeypatch, big)
    opt = v.default_options()
    cfg = v.workload.config(200, 80)
    ctx = _bench_ctx(4, cfg, v.workload.steady_point_obs(cfg))
    Bs, n_prior = v.workload.steady_batch(ctx, [0, 1, 2, 3], cfg, opt, chain=3)
    assert n_prior == 75
    ctx.solve()
    ctx.synchronize()
    pri, rep = ctx.download()
    _report("steady state", _check_all(ctx, pri, 4, "steady", 75))
    ctx.close()


def _pointless(n_lines, idx):
    cfg = v.workload.config(0, n_lines)
    cfg.track_len = 6
    return v.workload.generate(v.workload.seed_for(6, 8100 + idx), cfg, 0.3)


CAPS = {"default": (256, 128), "100,12": (100, 12), "48,24": (48, 24)}


@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("cap", list(CAPS))
def test_k_marg_on_windows_without_points(monkeypatch, big, cap):
    """a window without points (5 or 24 lines, one window per batch) on contexts of three capacities,
    fresh and behind a full-rank batch of another shape -- the kept block is all but constant, the factorisation stops at a
    rank < n.  (24 lines do not fit the context of 12: that pairing does not exist.)"""
    _set_big(monkeypatch, big)
    opt = v.default_options()
    P, L = CAPS[cap]
    mk = lambda: v.Context(device=0, max_windows=2, max_points=P, max_point_obs=P * 11, max_lines=L, max_line_obs=L * 11)
    cfgF = v.workload.config(40, 12)
    full = [v.workload.generate(v.workload.seed_for(3, 8200 + i), cfgF, 0.2 * i) for i in range(2)]
    wins = [_pointless(nl, k) for k, nl in enumerate((5, 24)) if nl <= L]
    c0 = mk()
    v.workload.set_preintegrations(full + wins, c0.preintegrate(*v.workload.imu_batch_arrays(full + wins), opt))
    c0.close()
    rows = []
    for k, w in enumerate(wins):
        fresh = mk()
        pf, _ = fresh.solve_windows([w.copy()], opt)
        rows += _check_all(fresh, pf, 1, (cap, "fresh", k))
        Jf, rf, nf = pf[0].J().copy(), pf[0].r().copy(), pf[0].n
        fresh.close()
        lived = mk()
        pl0, _ = lived.solve_windows([x.copy() for x in full], opt)
        pl, _ = lived.solve_windows([w.copy()], opt)
        rows += _check_all(lived, pl, 1, (cap, "long-lived", k))
        assert pl[0].n == nf and pl[0].J().tobytes() == Jf.tobytes() and pl[0].r().tobytes() == rf.tobytes(), (cap, k)
        lived.close()
    _report("no points, capacity %s" % cap, rows)


# ---- batches of mixed kept size ---------------------------------------------------------------------------------------------
# MARGIN_OLD without a prior keeps 15 + 6 (k - 1) dims, k = the length of the tracks that start in frame 0
MIXED_P, MIXED_L = 40, 12


def _mixed_ctx(nw=2):
    return v.Context(device=0, max_windows=nw, max_points=MIXED_P, max_point_obs=MIXED_P * 11, max_lines=MIXED_L,
                     max_line_obs=MIXED_L * 11)


def _mixed_windows(ctx, track_lens, opt):
    wins = []
    for k, tl in enumerate(track_lens):
        cfg = v.workload.config(MIXED_P, MIXED_L)
        cfg.track_len = tl
        wins.append(v.workload.generate(v.workload.seed_for(3, 8300 + 16 * tl + k), cfg, 0.2 * k))
    v.workload.set_preintegrations(wins, ctx.preintegrate(*v.workload.imu_batch_arrays(wins), opt))
    return wins


def _marg_result(ctx, pri, m, nn, i, win):
    """everything vpl_ba_marginalize hands back for window i (win) of the call just made, its kept block, and the part of the
    linearisation that the marginalisation pass of k_lin writes and k_marg reads (lin_H, lin_g out of
    vpl_ba_debug_linearization: the camera block and the rows of the landmarks that start in frame 0; the pass leaves the rows
    of every other landmark as they were), as arrays"""
    A, b = _kept_block_raw(ctx, i)
    nb = pri[i].n_blocks
    x0 = np.array([list(pri[i].x0[k]) for k in range(nb)])
    lin = ctx.debug_linearization(i)
    nP = lin["n_points"]
    rows = list(range(171)) + [171 + p for p in range(nP) if win.point_start[p] == 0]
    for dl, l in enumerate(lin["line_index"]):
        if win.line_start[l] == 0:
            rows += [171 + nP + 4 * dl + a for a in range(4)]
    lin = {"H": lin["H"][np.ix_(rows, rows)], "g": lin["g"][rows]}
    return {"J0": pri[i].J(), "r0": pri[i].r(), "x0": x0, "m": np.array([int(m[i])]), "n": np.array([int(nn[i])]),
            "mg_A": A, "mg_b": b, "lin_H": lin["H"], "lin_g": lin["g"]}


def _differences(a, b):
    """outputs that are not bit for bit equal -> {name: (entries that differ, of, largest difference)}"""
    out = {}
    for k in a:
        if a[k].shape != b[k].shape:
            out[k] = ("shape", a[k].shape, b[k].shape)
        elif a[k].tobytes() != b[k].tobytes():
            x, y = a[k].astype(np.float64).ravel(), b[k].astype(np.float64).ravel()
            out[k] = (int((x.view(np.uint64) != y.view(np.uint64)).sum()), x.size, float(np.nanmax(np.abs(x - y))))
    return out


def _mixed_batch(ctx, track_lens, want_n, tag):
    """the batch, the reference checks on each of its windows, then each window in a batch of its own on the same context;
    -> per window, the outputs that differ from the window alone ({} if none): _differences"""
    opt = v.default_options()
    wins = _mixed_windows(ctx, track_lens, opt)
    pri, m, nn = ctx.marginalize(wins, opt, capi.MARGIN_OLD)
    assert [int(x) for x in nn] == list(want_n) and [pri[i].n for i in range(len(wins))] == list(want_n), (tag, list(nn))   # input condition
    _report("mixed kept sizes %s" % (tag,), _check_all(ctx, pri, len(wins), tag))
    together = [_marg_result(ctx, pri, m, nn, i, wins[i]) for i in range(len(wins))]
    diff = []
    for i, w in enumerate(wins):
        p1, m1, n1 = ctx.marginalize([w], opt, capi.MARGIN_OLD)
        _check_all(ctx, p1, 1, (tag, "alone", i), want_n[i])
        alone = _marg_result(ctx, p1, m1, n1, 0, w)
        diff.append(_differences(alone, together[i]))
    return diff


MIXED_SMALL = {"39,33": ((5, 4), (39, 33)), "33,39": ((4, 5), (33, 39))}


@pytest.mark.parametrize("order", list(MIXED_SMALL))
def test_k_marg_small_on_a_batch_of_mixed_kept_size(monkeypatch, order):
    """k_marg<256>: the window that keeps 33 dims addresses 77 168 B of LDS, the one that keeps 39 only 67 536 B.
    (The equality with the window alone also needs k_lin's line phase to lay a window's lanes out by the window's own
    longest line track, not the batch's: DESIGN.md section 6.)"""
    _set_big(monkeypatch, 0)
    ctx = _mixed_ctx()
    diff = _mixed_batch(ctx, *MIXED_SMALL[order], tag=("small", order))
    ctx.close()
    assert diff == [{}, {}], diff


def test_k_marg_small_on_mixed_kept_sizes_leaves_the_guard_pads_intact():
    """the same batches with 0xA5 behind every device array (VPL_DEBUG_GUARDS=1): closing the context reports no overrun"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_psd_factor as t
ctx = t._mixed_ctx()
diffs = [t._mixed_batch(ctx, *t.MIXED_SMALL[order], tag=("guards", order)) for order in t.MIXED_SMALL]
ctx.close()
print("guards ok")
assert diffs == [[{}, {}]] * len(diffs), diffs
""" % (os.path.dirname(here), here)
    env = dict(os.environ, VPL_DEBUG_GUARDS="1")
    env.pop("VPL_BA_MARG_BIG", None)
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=env, cwd=os.path.dirname(here))
    assert "guards ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


MIXED_BIG = {"69,57": ((10, 8), (69, 57)), "39,33": ((5, 4), (39, 33))}


@pytest.mark.parametrize("sizes", list(MIXED_BIG))
def test_k_marg_big_on_a_batch_of_mixed_kept_size(monkeypatch, capsys, sizes):
    """k_marg<512> (by the kept size, or VPL_BA_MARG_BIG=1 for the sizes the 256-thread form would take): at 57 dims a window
    addresses 146 416 B, at 69 dims 137 520 B.  Equality with the window alone is asserted for n <= 48 and printed for both
    (also in a run without -s; profiles/r15/README.md keeps the lines of the runs made for it), the linearisation's for both:
    windows with the column-slice factorisation do not repeat their bits from run to run."""
    _set_big(monkeypatch, 1)
    ctx = _mixed_ctx()
    diff = _mixed_batch(ctx, *MIXED_BIG[sizes], tag=("big", sizes))
    ctx.close()
    with capsys.disabled():      # (the line is part of the suite's output also when it runs without -s)
        print("\nkept sizes %s on 512 threads: outputs that differ from the window alone (entries, of, largest): %s" % (sizes, diff))
    # the linearisation is k_lin's, the same for every kept size: a window's sums do not depend on the batch
    assert all("lin_H" not in d and "lin_g" not in d for d in diff), diff
    if max(MIXED_BIG[sizes][1]) <= 48:
        assert diff == [{}, {}], diff
