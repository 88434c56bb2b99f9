"""The pivoted Cholesky rule of csrc/ba_psd.h restated in plain NumPy, the crafted matrices it is tried on and the checks a
factor has to meet -- shared by tests/test_psd_factor_reference.py (CPU) and tests/test_gpu_psd_factor.py.

The rule (header comment of psd_pivoted_cholesky and of its one-wave form): P A P^T = L L^T with diagonal pivoting; the pivot
is the largest live diagonal, the lowest index on ties; tol = max(abs_tol, max(n eps, rel_tol) * first pivot); the
factorisation stops at the first pivot not above tol and the trailing block counts as zero; a right-hand side rides along
(L y = (P b)(0:rank)); positions rank..n-1 of perm are the indices that never were pivots, ascending.  k_marg writes the prior as
J0[k][perm[t]] = L[t][k], r0 = y, rows rank..n-1 zero.

No bound in here is taken from what the device computes: see check_factor."""
import numpy as np

EPS = 2.220446049250313e-16          # the double-precision eps of the rule's n eps term
LD = np.longdouble


class Ref:
    """rank, perm, L (n x rank, row t = original index perm[t]), y, pivots, S = the largest absolute entry of the trailing
    block at the stop, tol; cand[k] = (winner, runner-up) diagonals of step k (the rejected step included), dmax[k]"""


def pivoted_cholesky(A, b, abs_tol, rel_tol, dtype=LD, reciprocal=False, stop_scale=1):
    """dtype=longdouble: the reference.  dtype=float64, reciprocal=True: the device's form of the arithmetic (scaling by
    1 / sqrt(pivot)) in plain double, for the CPU test of the bounds.  stop_scale: the factorisation goes on down to
    stop_scale * tol (rank_window); S_at[k] is the largest entry of the trailing block had it stopped at rank k."""
    n = A.shape[0]
    W = np.array(A, dtype=dtype)
    c = np.array(b, dtype=dtype)
    alive = np.ones(n, dtype=bool)
    order, piv, cand, S_at = [], [], [], []
    L = np.zeros((n, n), dtype=dtype)
    y = np.zeros(n, dtype=dtype)
    tol = None
    idx = np.arange(n)
    while True:
        live = idx[alive]
        if live.size == 0:
            break
        d = W[live, live]
        p = int(live[int(np.argmax(d))])          # argmax returns the first maximum: the lowest index
        dp = W[p, p]
        if tol is None:
            tol = max(dtype(abs_tol), max(dtype(n * EPS), dtype(rel_tol)) * dp)
        rest = np.delete(d, int(np.argmax(d)))
        cand.append((dp, rest.max() if rest.size else None, np.abs(d).max()))
        S_at.append(np.abs(W[np.ix_(live, live)]).max())
        if not (dp > tol * stop_scale):
            break
        k = len(order)
        lkk = np.sqrt(dp)
        if reciprocal:
            inv = dtype(1.0) / lkk
            colv = W[:, p] * inv
            yk = c[p] * inv
        else:
            colv = W[:, p] / lkk
            yk = c[p] / lkk
        colv[~alive] = 0
        colv[p] = lkk
        L[:, k] = colv
        y[k] = yk
        alive[p] = False
        upd = idx[alive]
        W[np.ix_(upd, upd)] -= np.outer(colv[upd], colv[upd])
        c[upd] -= colv[upd] * yk
        order.append(p)
        piv.append(dp)
    r = Ref()
    r.rank = len(order)
    tail = idx[alive]
    r.perm = np.array(order + list(tail), dtype=np.int64)
    r.L = L[r.perm][:, : r.rank]
    r.y = y[: r.rank]
    r.pivots = np.array(piv, dtype=dtype)
    r.S = dtype(np.abs(W[np.ix_(tail, tail)]).max()) if tail.size else dtype(0)
    r.tol = tol if tol is not None else dtype(abs_tol)
    r.cand = cand
    r.S_at = S_at + [dtype(0)] * (n + 1 - len(S_at))
    return r


def rank_window(A, b, abs_tol, rel_tol):
    """For matrices that do not keep their pivots away from tol (the kept blocks of real windows): the rank may lie between
    the number of reference pivots above 10 tol and the number above tol / 10 -> (lo, hi, the largest S over that range)"""
    ref = pivoted_cholesky(A, b, abs_tol, rel_tol, stop_scale=0.1)
    lo = int((ref.pivots > 10 * ref.tol).sum())
    hi = int((ref.pivots > ref.tol / 10).sum())
    return lo, hi, max(ref.S_at[lo: hi + 1]), ref


def prior_of(ref, n):
    """J0, r0 in k_marg's layout out of a Ref (in its dtype)"""
    J = np.zeros((n, n), dtype=ref.L.dtype)
    for k in range(ref.rank):
        J[k, ref.perm] = ref.L[:, k]
    r0 = np.zeros(n, dtype=ref.L.dtype)
    r0[: ref.rank] = ref.y
    return J, r0


# ---- the cases ----------------------------------------------------------------------------------------------------------
N_WAVE16 = (1, 2, 15, 16)
N_WAVE48 = (1, 2, 15, 16, 17, 47, 48)
N_WAVE4 = (1, 2, 19, 20, 48, 49, 57, 64, 65, 75, 76)
N_WORKGROUP = tuple(sorted(set(N_WAVE16 + N_WAVE48 + N_WAVE4 + (77, 80))))
ABS_TOL = 1e-8                       # k_marg's kMargEps
REL_TOL_DEFICIENT = 1e-9             # rank-deficient cases: the stop must not hang on the rounding of the trailing block


class Case:
    def __init__(self, name, A, b, abs_tol, rel_tol, tie=None):
        self.name, self.A, self.b, self.abs_tol, self.rel_tol, self.tie = name, A, b, abs_tol, rel_tol, tie
        self.n = A.shape[0]


def _seed(*k):
    return np.random.default_rng([20260, *k])


def _ranks(n):
    return sorted({1, n // 2, n - 1, n} - {0})      # (target rank 0 is the zero matrix)


def _low_rank(kind, n, r):
    g = _seed(0 if kind == "integer" else 1, n, r)
    if kind == "integer":
        X = g.integers(-3, 4, size=(n, r)).astype(np.float64)
    else:
        X = g.standard_normal((n, r)) * np.logspace(0, -2, r)
    A = X @ X.T
    A = 0.5 * (A + A.T)
    return A, g.standard_normal(n)


def _tie(n, i, j):
    g = _seed(2, n, i, j)
    X = g.integers(-3, 4, size=(n, n)).astype(np.float64)
    A = X @ X.T + 5.0 * np.eye(n)
    top = A.diagonal().max() + 10.0
    A[i, i] = A[j, j] = top
    assert not np.array_equal(np.delete(A[i], [i, j]), np.delete(A[j], [i, j]))
    return A, g.standard_normal(n)


TIES = {16: [(3, 9)], 48: [(10, 40)], 75: [(63, 64), (5, 60)], 76: [(63, 64), (5, 60), (64, 70), (20, 70)], 80: [(63, 64), (70, 79)]}


def cases_for(sizes):
    out = []
    for n in sizes:
        g = _seed(3, n)
        out.append(Case("zero n=%d" % n, np.zeros((n, n)), g.standard_normal(n), ABS_TOL, 0.0))
        Xn = g.integers(-3, 4, size=(n, n)).astype(np.float64)
        An = Xn + Xn.T
        An[np.diag_indices(n)] = -np.abs(g.integers(0, 4, size=n)).astype(np.float64)
        An[n // 2, n // 2] = 0.0                  # (the largest diagonal is 0: the rounding term of the factor bound is 0, not negative)
        out.append(Case("diagonals <= 0 n=%d" % n, An, g.standard_normal(n), ABS_TOL, 0.0))
        out.append(Case("constant 7.5e8 n=%d" % n, np.full((n, n), 7.5e8), 1e4 * g.standard_normal(n), ABS_TOL, REL_TOL_DEFICIENT))
        for kind in ("integer", "graded"):
            for r in _ranks(n):
                A, b = _low_rank(kind, n, r)
                out.append(Case("%s n=%d r=%d" % (kind, n, r), A, b, ABS_TOL, 0.0 if r == n else REL_TOL_DEFICIENT))
        for (i, j) in TIES.get(n, []):
            A, b = _tie(n, i, j)
            out.append(Case("tie %d=%d n=%d" % (i, j, n), A, b, ABS_TOL, 0.0, tie=(i, j)))
    return out


def check_input_condition(case, ref):
    """every accepted pivot and the first rejected diagonal a factor 10 away from tol; the winner of every accepting step above
    the runner-up by more than 1e3 n eps max diag -- except an exact tie of step 0, where the entries are the caller's own
    (exact in every format) and the lowest index has to win.  A failure here is a mistake in the case list."""
    n = case.n
    tol = ref.tol
    for k, (win, second, dmax) in enumerate(ref.cand):
        if k < ref.rank:
            assert win >= 10 * tol, (case.name, k, "pivot too close to tol", float(win), float(tol))
            if second is None:
                continue
            if k == 0 and win == second:
                continue
            assert win - second > 1e3 * n * EPS * dmax, (case.name, k, "winner too close to the runner-up", float(win), float(second))
        else:
            assert win <= tol / 10, (case.name, k, "rejected diagonal too close to tol", float(win), float(tol))
    if case.tie:
        assert ref.rank == n and ref.perm[0] == case.tie[0], case.name
        d = case.A.diagonal()
        assert d[case.tie[0]] == d[case.tie[1]] == d.max() and (d == d.max()).sum() == 2, case.name


def check_factor(A, b, rank, perm, J0, r0, rank_lo, rank_hi, S, ref_perm=None, tag=""):
    """The assertions of a factor (J0, r0 in k_marg's layout) of A, b.  rank_lo <= rank <= rank_hi; S: what a correct stop may
    leave behind (the largest entry of the reference's trailing block).  Every bar is derived:
      |A - J0^T J0|max <= S + 2 (n + 1) eps max_i a_ii      (Cholesky backward error with (|L||L|^T)_ij <= max diag)
      |L_r r0 - (P b)(0:rank)| <= (n + 2) eps |L_r| |r0|    (Higham's forward substitution bound, two ulps for the reciprocal)
    -> (observed / bar) of the two, the largest over the entries, for reporting."""
    n = A.shape[0]
    assert rank_lo <= rank <= rank_hi, (tag, "rank", rank, rank_lo, rank_hi)
    perm = np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(n)), (tag, "perm is no permutation", perm.tolist())
    if ref_perm is not None:
        assert np.array_equal(perm, ref_perm), (tag, "perm", perm.tolist(), np.asarray(ref_perm).tolist())
    assert not np.isnan(J0).any() and not np.isnan(r0).any(), (tag, "entries the kernel never wrote")
    assert np.all(J0[rank:] == 0.0) and np.all(r0[rank:] == 0.0), (tag, "rows rank.. not zero")
    dmax = A.diagonal().max()
    round_term = 2 * (n + 1) * EPS * dmax
    Jl = J0.astype(LD)
    err = np.abs(A.astype(LD) - Jl.T @ Jl).max() if n else 0
    bar = S + LD(round_term)
    assert err <= bar, (tag, "|A - J0^T J0|", float(err), float(bar))
    ratio, rratio = (float(err / bar) if bar > 0 and rank > 0 else 0.0), 0.0   # (rank 0: err = S, nothing to report)
    Lr = J0[:rank][:, perm[:rank]].T            # rank x rank, lower triangular
    assert np.all(np.triu(Lr, 1) == 0.0), (tag, "J0[k][perm[t]] != 0 for t < k")
    piv = np.diag(Lr)
    assert np.all(piv > 0), (tag, "pivots not positive")
    if rank > 1:
        assert np.all(piv[1:].astype(LD) ** 2 <= piv[:-1].astype(LD) ** 2 + LD(round_term)), (tag, "pivots increase")
    if rank:
        Ll, rl = Lr.astype(LD), r0[:rank].astype(LD)
        res = np.abs(Ll @ rl - b[perm[:rank]].astype(LD))
        rbar = (n + 2) * EPS * (np.abs(Ll) @ np.abs(rl))
        assert np.all(res <= rbar), (tag, "r0", float((res - rbar).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(rbar > 0, res / np.where(rbar > 0, rbar, 1), 0)
        rratio = float(q.max())
    return ratio, rratio
