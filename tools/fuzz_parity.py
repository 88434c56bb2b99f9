"""Randomised parity sweep (GPU box): the HIP solve against the oracle on windows whose SHAPE is drawn at random --
counts of points / lines, VP observations on or off, track lengths 2..11 (lines 5..11) trimmed per track, tracks dropped, lines marked
untriangulated, every marginalisation mode, extrinsic fixed or free, 1..8 iterations, with and without a prior from a preceding
window (one keyframe on with MARGIN_OLD; the same frames again with MARGIN_SECOND_NEW), several shapes in ONE batch.  Prints one line per window and a summary.

The bar is BASELINE.json's: 1e-4 m / 1e-6 rad and the oracle's iteration / accepted-step counts.  Shapes drawn at random include
windows that do not determine their states to that accuracy (one point and five lines; a prior whose weak eigenvalues sit
next to the reference's 1e-8 cut while the IMU rows of the marginalisation carry entries of 5e14): there the ORACLE does not
reproduce itself under changes that are rounding and nothing else.  Every window is therefore solved by the oracle four times:
as drawn; with the initial positions of the frames moved by 1e-10 m each and every inverse depth and Pluecker coordinate
by 1e-10 of itself (at random); and with the products of the
marginalisation's Schur complements summed differently (oracle/marginalization.cpp, g_marg_reverse_sums: 1 = the last one's
inner sums backwards, 2 = both accumulated in long double and rounded once: the same terms, another rounding -- for a
chained window the first solve runs with the switch and hands its prior on).  `sens` is the largest distance of a variant
from the first answer.  The device differs from the oracle in the order of EVERY sum, not of
one: a window outside the bar counts as a MISS only if the device is more than ten times further from the oracle than the
oracle is from itself; otherwise it is printed as `ill-posed`.  Exit status 1 if there is a MISS.

    python tools/fuzz_parity.py [batches=12] [windows per batch=8] [seed=1] [prior rule: 0 pivoted Cholesky (default), 1 eigen]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C

import numpy as np

import oracle_api as o
import vplines_slam_amd as v
from vplines_slam_amd.capi import Prior, Window

NF = 11
POS_TOL, ROT_TOL = 1e-4, 1e-6
MARGIN = 10.0            # see the header
LIB = o.load()
LIB.orc_set_marg_reverse_sums.argtypes = [C.c_int]


def pose_err(a, b, _=None):
    dp = np.linalg.norm(a.pose[:, :3] - b.pose[:, :3], axis=1).max()
    qa, qb = a.pose[:, 3:], b.pose[:, 3:]
    dots = np.clip(np.abs((qa * qb).sum(1)) / (np.linalg.norm(qa, axis=1) * np.linalg.norm(qb, axis=1)), 0, 1)
    return dp, (2 * np.arccos(dots)).max()


# FUZZ_CAPS="P,L": contexts of another capacity than the default 256 points / 128 lines (strides, LDS windows and the choice
# between kernel variants depend on it); the shapes drawn stay within it and include it
CAP_P, CAP_L = (int(x) for x in os.environ.get("FUZZ_CAPS", "256,128").split(","))


def make_ctx(per):
    return v.Context(device=0, max_windows=per, max_points=CAP_P, max_point_obs=CAP_P * 11, max_lines=CAP_L, max_line_obs=CAP_L * 11)


def draw_window(rng, idx, t):
    P = int(rng.choice([x for x in (0, 1, 3, 17, 64, 150, 200, 256) if x < CAP_P] + [CAP_P]))
    L = int(rng.choice([x for x in (0, 1, 5, 33, 80, 128) if x < CAP_L] + [CAP_L]))
    if P == 0 and L == 0:
        P = min(40, CAP_P)
    vp = bool(rng.integers(0, 2))
    cfg = v.workload.config(P, L, vp)
    # the window holds the tracks that pass the reference's filters (include/vplines_ba.h): points with >= 2 observations,
    # lines with >= LINE_MIN_OBS = 5 (parameters.h:23) -- a line seen twice has one 2-row factor for 4 degrees of freedom
    cfg.track_len = int(rng.choice([5, 6, 6, 6, 8, 11] if L else [2, 3, 4, 6, 6, 6, 8, 11]))
    w = v.workload.generate(v.workload.seed_for(6, idx), cfg, t)
    TL = cfg.track_len
    # trim tracks from the end (the start frame carries the inverse depth / the Pluecker line), drop some altogether
    def trim(start, nobs, obs, per_track, width, least):
        off = np.concatenate([[0], np.cumsum(nobs)])
        keep, ns, nn, no, kept = [], [], [], [], []
        for k in range(len(start)):
            r = rng.random()
            if r < 0.08:
                continue
            n = int(nobs[k])
            if r < 0.45 and n > least:
                n = int(rng.integers(least, n + 1))
            ns.append(start[k]); nn.append(n); no.append(obs[off[k]:off[k] + n]); kept.append(k)
        obs2 = np.concatenate(no) if no else np.zeros((0, width))
        return np.array(ns, np.int32), np.array(nn, np.int32), obs2, [per_track[k] for k in kept]
    ps, pn, po, invd = trim(w.point_start, w.point_nobs, w.point_obs, list(w.inv_depth), 3, 2)
    ls, ln, lo, plk = trim(w.line_start, w.line_nobs, w.line_obs, list(w.line_plk), 8, 5)
    r = Window(w.pose, w.speed_bias, w.ex_pose, ps, pn, po, np.array(invd), ls, ln, lo,
               np.array(plk).reshape(-1, 6) if plk else np.zeros((0, 6)))
    r.extra = dict(w.extra)
    if len(ls):
        r.line_triangulated[:len(ls)] = (rng.random(len(ls)) > 0.1).astype(np.int32)
    return r, (P, L, vp, TL)


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    res = run(nb, per, int(sys.argv[3]) if len(sys.argv) > 3 else 1, prior_rule=int(sys.argv[4]) if len(sys.argv) > 4 else None)
    return 1 if res["miss"] else 0


def run(nb, per, seed, out=print, prior_rule=None):
    """-> dict(total, miss, ill, miss_first, total_first, worst_dp, worst_dr); *_first count the windows solved without an
    incoming prior (the chained ones depend on the marginalisation of the solve before).  prior_rule: vpl_ba_set_prior_rule
    on the device's context (None: the context's default)"""
    rng = np.random.default_rng(seed)
    ctx = make_ctx(per)
    if prior_rule is not None:
        ctx.set_prior_rule(prior_rule)
    bad = total = ill = bad0 = total0 = 0
    worst = [0.0, 0.0]                                # over the windows that determine their states
    for b in range(nb):
        opt = v.default_options()
        opt.num_iterations = int(rng.choice([1, 2, 3, 5, 5, 8]))
        opt.estimate_extrinsic = int(rng.integers(0, 2))
        opt.marginalization_flag = int(rng.choice([v.MARGIN_OLD, v.MARGIN_OLD, v.MARGIN_SECOND_NEW, v.MARGIN_NONE]))
        chained = opt.marginalization_flag != v.MARGIN_NONE and rng.random() < 0.5
        ws, shapes = [], []
        for i in range(per):
            w, sh = draw_window(rng, 1000 * b + i, 0.37 * (b * per + i))
            ws.append(w); shapes.append(sh)
        o.preintegrate_windows(ws, opt)
        wg, wc = [w.copy() for w in ws], [w.copy() for w in ws]
        try:
            pg, rg = ctx.solve_windows(wg, opt)
        except Exception as e:                       # a refusal is a result too: print the shapes
            out("batch %d REFUSED: %s  shapes %s" % (b, e, shapes)); bad += 1; bad0 += 1
            continue
        pcs, pcs_s, pcs_r = [], [], []
        for i in range(per):
            pc, rc = o.solve_window(wc[i], opt)
            pcs.append(pc)
            ws_s = shifted(ws[i])
            pc_s, _ = o.solve_window(ws_s, opt)
            pcs_s.append(pc_s)
            pr = []
            for mode in (1, 2):
                LIB.orc_set_marg_reverse_sums(mode)
                pr.append(o.solve_window(ws[i].copy(), opt)[0])     # (the states of this solve do not depend on the switch)
            LIB.orc_set_marg_reverse_sums(0)
            pcs_r.append(pr)
            line = report(b, i, shapes[i], opt, 0, wg[i], wc[i], rg[i], rc, pg[i], pc, pose_err(ws_s, wc[i], 1e-10), out)
            total += 1; bad += line[0]; ill += line[3]; worst = [max(worst[0], line[1]), max(worst[1], line[2])]
            total0 += 1; bad0 += line[0]
        if chained:
            # the same trajectories one keyframe later, each side carrying ITS OWN prior
            w2 = []
            for i in range(per):
                w, _ = draw_window(np.random.default_rng(7000 + 100 * b + i), 1000 * b + 500 + i, 0.37 * (b * per + i) + 0.1)   # + kf_dt: the window one keyframe on
                w2.append(w)
            o.preintegrate_windows(w2, opt)
            keep = (Prior * per)()
            C.memmove(keep, pg, C.sizeof(keep))
            # the device-resident hand-over first (vpl_ba_upload_chained needs the solve above to be the context's last upload):
            # the same windows, the priors never leaving the device -- must give the bits of the host hand-over below
            gd = [w.copy() for w in w2]
            ctx.upload(gd, opt, chained=True)
            ctx.solve()
            ctx.synchronize()
            ctx.download()
            g2, c2 = [w.copy() for w in w2], [w.copy() for w in w2]
            for i in range(per):
                g2[i].prior = keep[i] if keep[i].n > 0 else None
                c2[i].prior = pcs[i] if pcs[i].n > 0 else None
            pg2, rg2 = ctx.solve_windows(g2, opt)
            for i in range(per):
                if not (np.array_equal(gd[i].pose, g2[i].pose) and np.array_equal(gd[i].speed_bias, g2[i].speed_bias)):
                    out("b%02d.1 w%d CHAINED UPLOAD differs from the host hand-over: %.3e <-- MISS" % (
                        b, i, np.abs(gd[i].pose - g2[i].pose).max()))
                    bad += 1
            for i in range(per):
                pc, rc = o.solve_window(c2[i], opt)
                c2s = shifted(w2[i])
                c2s.prior = pcs_s[i] if pcs_s[i].n > 0 else None
                o.solve_window(c2s, opt)
                sa, sb = pose_err(c2s, c2[i]), (0.0, 0.0)
                for prv in pcs_r[i]:
                    c2r = w2[i].copy()
                    c2r.prior = prv if prv.n > 0 else None
                    o.solve_window(c2r, opt)
                    e = pose_err(c2r, c2[i])
                    sb = (max(sb[0], e[0]), max(sb[1], e[1]))
                line = report(b, i, ("chained",), opt, 1, g2[i], c2[i], rg2[i], rc, pg2[i], pc,
                              (max(sa[0] - 1e-10 * np.sqrt(3.0), sb[0]) + 1e-10 * np.sqrt(3.0), max(sa[1], sb[1])), out)
                total += 1; bad += line[0]; ill += line[3]; worst = [max(worst[0], line[1]), max(worst[1], line[2])]
        if opt.marginalization_flag == v.MARGIN_OLD and not chained:
            # MARGIN_SECOND_NEW behind a prior: the same frames again (another draw of the noise and of the tracks) with the
            # prior of the first solve; the second-newest frame leaves (estimator.cpp:1385-1453)
            opt3 = v.default_options()
            opt3.num_iterations, opt3.estimate_extrinsic = opt.num_iterations, opt.estimate_extrinsic
            opt3.marginalization_flag = v.MARGIN_SECOND_NEW
            w3 = []
            for i in range(per):
                w, _ = draw_window(np.random.default_rng(9000 + 100 * b + i), 1000 * b + 700 + i, 0.37 * (b * per + i))
                w3.append(w)
            o.preintegrate_windows(w3, opt3)
            keep = (Prior * per)()
            C.memmove(keep, pg, C.sizeof(keep))
            g3, c3 = [w.copy() for w in w3], [w.copy() for w in w3]
            for i in range(per):
                g3[i].prior = keep[i] if keep[i].n > 0 else None
                c3[i].prior = pcs[i] if pcs[i].n > 0 else None
            pg3, rg3 = ctx.solve_windows(g3, opt3)
            for i in range(per):
                pc, rc = o.solve_window(c3[i], opt3)
                sa, sb = (0.0, 0.0), (0.0, 0.0)
                c3s = shifted(w3[i]); c3s.prior = pcs_s[i] if pcs_s[i].n > 0 else None
                o.solve_window(c3s, opt3); sa = pose_err(c3s, c3[i])
                for prv in pcs_r[i]:
                    c3r = w3[i].copy(); c3r.prior = prv if prv.n > 0 else None
                    o.solve_window(c3r, opt3)
                    e = pose_err(c3r, c3[i]); sb = (max(sb[0], e[0]), max(sb[1], e[1]))
                line = report(b, i, ("second-new",), opt3, 2, g3[i], c3[i], rg3[i], rc, pg3[i], pc,
                              (max(sa[0] - 1e-10 * np.sqrt(3.0), sb[0]) + 1e-10 * np.sqrt(3.0), max(sa[1], sb[1])), out)
                total += 1; bad += line[0]; ill += line[3]; worst = [max(worst[0], line[1]), max(worst[1], line[2])]
    ctx.close()
    out("fuzz_parity: %d windows, %d MISS, %d ill-posed (outside the bar, within 10 x the oracle's distance from itself); "
        "worst of the others dp %.2e m dr %.2e rad; without an incoming prior: %d windows, %d MISS"
        % (total, bad, ill, worst[0], worst[1], total0, bad0))
    return dict(total=total, miss=bad, ill=ill, total_first=total0, miss_first=bad0, worst_dp=worst[0], worst_dr=worst[1])


def shifted(w, d=1e-10):
    """every frame's initial position moved by its own offset of up to d per axis (a common offset would be a gauge
    motion: the answer moves with it and nothing is learnt)"""
    s = w.copy()
    r = np.random.default_rng(12345)
    s.pose[:, :3] += d * r.uniform(-1.0, 1.0, (NF, 3))
    # ... and the landmarks by the same relative amount: a window whose lines are barely determined keeps its poses to 1e-9
    # through several iterations while the line parameters (and with them the cost, then an accept / reject decision) drift
    if len(s.inv_depth):
        s.inv_depth *= 1.0 + d * r.uniform(-1.0, 1.0, len(s.inv_depth))
    if len(s.line_plk):
        s.line_plk *= 1.0 + d * r.uniform(-1.0, 1.0, s.line_plk.shape)
    return s


def report(b, i, shape, opt, stage, wg, wc, rg, rc, pg, pc, sens, out=print):
    dp, dr = pose_err(wg, wc)
    sp, sr = sens[0] - 1e-10 * np.sqrt(3.0), sens[1]     # (the shift itself is not sensitivity)
    ok = (rg.iterations == rc.iterations and rg.num_successful_steps == rc.num_successful_steps and dp <= POS_TOL and dr <= ROT_TOL
          and pg.n == pc.n)
    illp = (not ok) and pg.n == pc.n and dp <= max(POS_TOL, MARGIN * sp) and dr <= max(ROT_TOL, MARGIN * sr)
    out("b%02d.%d w%d %-22s it%d ex%d mg%+d  iter %d/%d succ %d/%d prior %d/%d cost %.6e/%.6e dp %.1e dr %.1e sens %.1e %.1e %s" % (
        b, stage, i, str(shape), opt.num_iterations, opt.estimate_extrinsic, opt.marginalization_flag, rg.iterations, rc.iterations,
        rg.num_successful_steps, rc.num_successful_steps, pg.n, pc.n, rg.final_cost, rc.final_cost, dp, dr, max(sp, 0.0), sr,
        "" if ok else ("ill-posed" if illp else "<-- MISS")))
    return (0 if ok or illp else 1), (0.0 if illp else dp), (0.0 if illp else dr), (1 if illp else 0)


if __name__ == "__main__":
    sys.exit(main())
