"""tests/firth_reference.py against what is known in closed form, and its own rounding error.

The closed forms (one parameter per cell): Firth's logistic fit has pi_g = (S_g + 1/2) / (n_g + 1), the Poisson / log
fit mu_g = (S_g + 1/2) / n_g, finite in cells of all successes, all failures or all zeros; sum h = p at any beta.
For the canonical links g* is the gradient of l(beta) + log det(X'WX) / 2.
"""
import numpy as np
import pytest

import firth_reference as F
from conftest import nrel
from sandwich_reference import scaled_err


def cell_design(counts):
    ids = np.repeat(np.arange(len(counts)), counts)
    X = np.zeros((len(ids), len(counts)), order="F")
    X[np.arange(len(ids)), ids] = 1.0
    return X, ids


def test_logistic_cells_have_the_closed_form():
    """pi_g = (S_g + 1/2) / (n_g + 1), with a cell of all successes and one of all failures."""
    n_g, S_g = np.array([10, 7, 12, 9, 6]), np.array([3, 7, 0, 4, 5])
    X, ids = cell_design(n_g)
    y = np.concatenate([np.r_[np.ones(s), np.zeros(n - s)] for n, s in zip(n_g, S_g)])
    o = F.firth_fit(X, y, "binomial", "logit", epsilon=1e-12)
    pi = 1.0 / (1.0 + np.exp(-o["coefs"]))
    err = np.max(np.abs(pi - (S_g + 0.5) / (n_g + 1.0)))
    print(f"\nlogistic cells: max |pi - closed form| {err:.2e}, {o['iter']} iterations, sum h {o['sum_hat']!r}")
    assert o["converged"] and err <= 1e-10
    assert abs(o["sum_hat"] - 5) <= 5e-12


def test_separated_two_by_two_table_has_a_finite_slope():
    """3 / 10 against 7 / 7: the slope is logit(7.5 / 8) - logit(3.5 / 11) = 3.4702."""
    x = np.r_[np.zeros(10), np.ones(7)]
    X = np.asfortranarray(np.c_[np.ones(17), x])
    y = np.r_[np.ones(3), np.zeros(7), np.ones(7)]
    o = F.firth_fit(X, y, "binomial", "logit", epsilon=1e-12)
    lg = lambda q: np.log(q / (1 - q))
    want = np.array([lg(3.5 / 11), lg(7.5 / 8) - lg(3.5 / 11)])
    assert o["converged"] and np.max(np.abs(o["coefs"] - want)) <= 1e-10
    assert abs(want[1] - 3.4702) < 5e-5


def test_poisson_cells_have_the_closed_form():
    """mu_g = (S_g + 1/2) / n_g, with a cell of all zeros."""
    n_g = np.array([6, 9, 5, 8])
    rng = np.random.default_rng(5)
    y = rng.poisson(3.0, n_g.sum()).astype(np.float64)
    X, ids = cell_design(n_g)
    y[ids == 1] = 0.0
    S_g = np.bincount(ids, weights=y)
    o = F.firth_fit(X, y, "poisson", "log", epsilon=1e-12)
    err = np.max(np.abs(np.exp(o["coefs"]) - (S_g + 0.5) / n_g))
    print(f"\npoisson cells: max |mu - closed form| {err:.2e}, {o['iter']} iterations")
    assert o["converged"] and err <= 1e-10
    assert abs(o["sum_hat"] - 4) <= 4e-12


@pytest.mark.parametrize("fam,lnk", F.PAIRS)
def test_the_leverages_sum_to_p_at_every_iterate(fam, lnk):
    c = F.make_case(fam, lnk, 700, 6, 3)
    kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
    for k in range(4):
        o = F.firth_fit(c["X"], c["y"], fam, lnk, maxit=k, **kw)
        assert o["iter"] == k and abs(o["sum_hat"] - 6) <= 6e-12, (k, o["sum_hat"])


def penalized_loglik(X, y, beta, fam, m, off, pw):
    """l(beta) + log det(X'WX) / 2 of the two canonical pairs in np.longdouble (the constants in y dropped)."""
    ld = np.longdouble
    Xd, eta = X.astype(ld), X.astype(ld) @ beta.astype(ld) + off.astype(ld)
    if fam == "binomial":
        pi = 1 / (1 + np.exp(-eta))
        ll = np.sum(pw * (y * eta - m * np.log1p(np.exp(eta))))
        w = pw * m * pi * (1 - pi)
    else:
        ll = np.sum(pw * (y * eta - np.exp(eta)))
        w = pw * np.exp(eta)
    A = Xd.T @ (w.astype(ld)[:, None] * Xd)
    logdet = ld(0)
    for i in range(A.shape[0]):  # unpivoted elimination: the sum of the log pivots
        logdet += np.log(A[i, i])
        f = A[i + 1:, i] / A[i, i]
        A[i + 1:, i:] -= f[:, None] * A[i, i:][None, :]
    return ll + logdet / 2


@pytest.mark.parametrize("fam,lnk", [("binomial", "logit"), ("poisson", "log")])
def test_the_adjusted_score_is_the_gradient_of_the_penalized_likelihood(fam, lnk):
    c = F.make_case(fam, lnk, 300, 5, 4)
    m = np.ones(300) if c["m"] is None else c["m"]
    beta = c["beta"] * 0.7
    g = F.firth_pass(c["X"], c["y"], beta, fam, lnk, m=c["m"], off=c["off"], pw=c["pw"])["g"]
    fd = np.zeros(5)
    step = np.longdouble(1e-5)
    for j in range(5):
        e = np.zeros(5, dtype=np.longdouble)
        e[j] = step
        b = beta.astype(np.longdouble)
        fd[j] = float((penalized_loglik(c["X"], c["y"], b + e, fam, m, c["off"], c["pw"]) -
                       penalized_loglik(c["X"], c["y"], b - e, fam, m, c["off"], c["pw"])) / (2 * step))
    err = float(np.max(np.abs(g - fd) / np.max(np.abs(fd))))
    print(f"\n{fam}/{lnk}: g* against the finite-difference gradient {err:.2e}")
    assert err <= 1e-6


def test_the_identity_link_has_no_adjustment():
    """r = 0: the Firth fit of poisson / identity is the ML fit."""
    c = F.make_case("poisson", "identity", 900, 5, 5)
    kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
    o = F.firth_fit(c["X"], c["y"], "poisson", "identity", epsilon=1e-12, **kw)
    ml = F.ml_fit(c["X"], c["y"], "poisson", "identity", **kw)[-1]
    assert o["converged"] and np.max(np.abs(o["coefs"] - ml)) <= 1e-9 * np.max(np.abs(ml))


def separated_case(n=170):
    """The 3 / 10 against 7 / 7 table replicated: complete separation of the x = 1 rows."""
    k = n // 17
    x = np.r_[np.zeros(10 * k), np.ones(7 * k)]
    y = np.r_[np.ones(3 * k), np.zeros(7 * k), np.ones(7 * k)]
    return np.asfortranarray(np.c_[np.ones(17 * k), x]), y


def test_separation_diverges_under_ml_and_converges_under_firth():
    X, y = separated_case()
    ml = F.ml_fit(X, y, "binomial", "logit", iters=25)
    assert np.max(np.abs(ml[-1])) > 10.0
    o = F.firth_fit(X, y, "binomial", "logit")
    assert o["converged"] and np.max(np.abs(o["coefs"])) < 10.0 and o["iter"] < 25


@pytest.mark.parametrize("fam,lnk", [("binomial", "logit"), ("poisson", "log")])
def test_the_references_own_error(fam, lnk):
    """fp64 against np.longdouble and against the rows in reverse order at 1300 x 20: what the GPU tests' 1e-9
    bars can lose to the reference itself."""
    c = F.make_case(fam, lnk, 1300, 20, 6)
    kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
    beta = c["beta"] * 0.8
    a = F.firth_pass(c["X"], c["y"], beta, fam, lnk, **kw)
    worst = 0.0
    for other in (F.firth_pass(c["X"], c["y"], beta, fam, lnk, dtype=np.longdouble, **kw),
                  F.firth_pass(c["X"], c["y"], beta, fam, lnk, reverse=True, **kw)):
        b = {k: np.asarray(v, dtype=np.float64) for k, v in other.items()}
        errs = dict(A=scaled_err(a["A"], b["A"]), g=nrel(a["g"], b["g"]),
                    sum_hat=abs(a["sum_hat"] - b["sum_hat"]) / 20, hat=float(np.max(np.abs(a["hat"] - b["hat"]))))
        print(f"\n{fam}/{lnk} reference error: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        worst = max(worst, *errs.values())
    assert worst <= 1e-11
