"""The reference of tests/test_gpu_psd_factor.py on its own (no GPU): the pivoted Cholesky rule restated in long double
(tests/psd_factor_ref.py) against the same restatement in plain double with the device's reciprocal-multiply arithmetic, on
exactly the GPU test's case list.  The double restatement must find the reference's rank and perm and stay inside the bars the
GPU test sets for the kernels; the input condition of the case list is asserted here too.  The margins are printed."""
import numpy as np
import pytest

import psd_factor_ref as R


@pytest.fixture(scope="module")
def cases():
    cs = R.cases_for(R.N_WORKGROUP)
    return [(c, R.pivoted_cholesky(c.A, c.b, c.abs_tol, c.rel_tol)) for c in cs]


def test_long_double_is_wider_than_double():
    assert np.finfo(R.LD).eps < 1e-18, "numpy.longdouble is no wider than double here: the reference would prove nothing"


def test_case_list_covers_the_issue(cases):
    names = [c.name for c, _ in cases]
    assert len(set(names)) == len(names)
    for n in R.N_WORKGROUP:
        got = {ref.rank for c, ref in cases if c.n == n}
        assert got >= {0, 1, n // 2, n - 1, n}, (n, got)
    for forms in (R.N_WAVE16, R.N_WAVE48, R.N_WAVE4):
        assert set(forms) <= set(R.N_WORKGROUP)
    ties = [c for c, _ in cases if c.tie]
    assert any(c.tie == (63, 64) for c in ties) and any(c.tie[1] < 64 for c in ties) and any(c.tie[0] >= 64 for c in ties)


def test_input_condition_holds_for_every_case(cases):
    for c, ref in cases:
        R.check_input_condition(c, ref)


def test_reference_ranks_are_the_constructed_ones(cases):
    for c, ref in cases:
        if c.name.startswith(("integer", "graded")):
            assert ref.rank == int(c.name.split("r=")[1]), c.name
        elif c.name.startswith(("zero", "diagonals")):
            assert ref.rank == 0 and np.array_equal(ref.perm, np.arange(c.n)), c.name
        elif c.name.startswith("constant"):
            assert ref.rank == 1 and ref.perm[0] == 0, c.name


def test_reference_meets_its_own_bars(cases):
    """the long double factor itself, rounded to double, and the rule in plain double"""
    worst = {"long double": [0.0, 0.0], "double": [0.0, 0.0]}
    for c, ref in cases:
        J, r0 = R.prior_of(ref, c.n)
        q = R.check_factor(c.A, c.b, ref.rank, ref.perm, J.astype(np.float64), r0.astype(np.float64), ref.rank, ref.rank, ref.S,
                           ref.perm, ("long double", c.name))
        worst["long double"] = [max(a, b) for a, b in zip(worst["long double"], q)]
        dbl = R.pivoted_cholesky(c.A, c.b, c.abs_tol, c.rel_tol, dtype=np.float64, reciprocal=True)
        assert dbl.rank == ref.rank and np.array_equal(dbl.perm, ref.perm), c.name
        J, r0 = R.prior_of(dbl, c.n)
        q = R.check_factor(c.A, c.b, dbl.rank, dbl.perm, J, r0, ref.rank, ref.rank, ref.S, ref.perm, ("double", c.name))
        worst["double"] = [max(a, b) for a, b in zip(worst["double"], q)]
    for k, (f, r) in worst.items():
        print("%s restatement over %d cases: at most %.3f of the factor bar, %.3f of the r0 bar" % (k, len(cases), f, r))
    assert max(worst["double"]) <= 1.0
