"""tests/multinom_reference.py against itself and against what it must reduce to: fp64 against np.longdouble and
against the rows in reverse order (the reference's own error), K = 2 against oracle/np_reference's binomial / logit
fit, the score against a central finite difference of the deviance, the null deviance's closed form against an
intercept-only fit.  No GPU.

The reference's own error as measured here at 2000 x 8 (K = 3) and 4001 x 33 (K = 4): H <= 5.2e-15 (scaled), g <=
4.1e-15, deviance <= 1.1e-16, P <= 1.2e-16 -- so the 1e-9 bars of tests/test_gpu_multinom.py keep > 1e5 of margin
from the reference alone.
"""
import numpy as np

import multinom_reference as M
import np_reference as R
from conftest import nrel, rel
from sandwich_reference import scaled_err


def test_own_error_against_longdouble_and_reverse_order():
    c = M.make_case(1300, 20, 4, 1)
    B = 0.8 * c["B"]
    a = M.multinom_pass(c["X"], c["y"], B, c["pw"])
    for label, kw in (("longdouble", dict(dtype=np.longdouble)), ("reverse", dict(reverse=True))):
        b = M.multinom_pass(c["X"], c["y"], B, c["pw"], **kw)
        f = lambda v: np.asarray(v, dtype=np.float64)
        errs = dict(H=scaled_err(a["H"], f(b["H"])), g=nrel(a["g"], f(b["g"])),
                    dev=rel(a["deviance"], float(b["deviance"])), P=float(np.max(np.abs(a["P"] - f(b["P"])))),
                    null=rel(a["null_deviance"], float(b["null_deviance"])))
        print(f"\nreference's own error ({label}): " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-11, (label, errs)
    assert scaled_err(a["H"].T, a["H"]) <= 1e-14
    assert np.all(a["R"][c["pw"] == 0] == 0.0) and np.any(c["pw"] == 0)


def test_k2_is_the_binomial_logit_fit():
    c = M.make_case(1500, 6, 2, 3)
    o = R.fit_glm(c["X"], c["y"], "binomial", "logit", prior=c["pw"], tol=1e-13)
    f = M.multinom_fit(c["X"], c["y"], 2, c["pw"], epsilon=1e-14)
    assert f["converged"] and f["halvings"] == 0
    errs = dict(coefs=rel(f["coefs"][0], o.coefs), stderr=rel(f["stderr"][0], o.stderr),
                dev=rel(f["deviance"], o.deviance))
    # (not the null deviance: the binomial fit's is taken at the unweighted mean of y, the reference's own rule,
    # the multinomial one at the weighted class shares -- test_null_deviance_is_the_intercept_only_fit)
    print(f"\nK = 2 against np_reference: {errs}")
    assert max(errs.values()) <= 1e-10, errs


def test_score_is_the_gradient_of_the_deviance():
    c = M.make_case(800, 5, 3, 4)
    B = 0.8 * c["B"]
    a = M.multinom_pass(c["X"], c["y"], B, c["pw"])
    h = 1e-5
    fd = np.zeros_like(a["g"])
    p = 5
    for idx in range(fd.size):
        j, col = divmod(idx, p)
        E = np.zeros_like(B)
        E[col, j] = h
        up = M.multinom_pass(c["X"], c["y"], B + E, c["pw"])["deviance"]
        dn = M.multinom_pass(c["X"], c["y"], B - E, c["pw"])["deviance"]
        fd[idx] = -(up - dn) / (4 * h)  # g = d loglik / d theta = -(dD / d theta) / 2
    # the central difference's own error: h^2 |D'''| / 6 ~ 1e-10 sum pw, and eps D / h ~ 1e-8
    assert np.max(np.abs(fd - a["g"])) <= 1e-6 * np.max(np.abs(a["g"])), (fd, a["g"])
    # and H is its negative Jacobian: one column by differences of g
    E = np.zeros_like(B)
    E[2, 1] = h
    gu = M.multinom_pass(c["X"], c["y"], B + E, c["pw"])["g"]
    gd = M.multinom_pass(c["X"], c["y"], B - E, c["pw"])["g"]
    col = -(gu - gd) / (2 * h)
    assert np.max(np.abs(col - a["H"][:, p + 2])) <= 1e-6 * np.max(np.abs(a["H"]))


def test_null_deviance_is_the_intercept_only_fit():
    c = M.make_case(900, 4, 5, 5)
    ones = np.ones((900, 1), order="F")
    f = M.multinom_fit(ones, c["y"], 5, c["pw"], epsilon=1e-14)
    full = M.multinom_pass(c["X"], c["y"], c["B"], c["pw"])
    assert f["converged"]
    assert rel(f["deviance"], full["null_deviance"]) <= 1e-12
    # its fitted probabilities are the weighted class shares
    P = M.rows(ones, c["y"], f["B"], c["pw"])["P"][0]
    assert rel(P, full["counts"] / full["sum_w"]) <= 1e-10


def test_fit_converges_quadratically_and_epsilon_is_clear():
    c = M.make_case(2000, 8, 3, 2)
    long = M.multinom_fit(c["X"], c["y"], 3, c["pw"], epsilon=1e-15, max_iter=12)
    eps = M.pick_epsilon(long["trace"])
    assert M.clearance(long["trace"], eps) >= 10.0, long["trace"]
    f = M.multinom_fit(c["X"], c["y"], 3, c["pw"], epsilon=eps)
    assert f["converged"] and 3 <= f["iter"] <= 7 and f["halvings"] == 0, (f["iter"], f["halvings"], long["trace"])
    assert np.linalg.cond(f["H"]) <= 1e3
