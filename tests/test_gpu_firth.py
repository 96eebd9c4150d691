"""Firth's bias-reduced fits on the GPU (sglm_fit_glm_firth, sglm_firth_pass: influence.hip's firth_kernel, and past
the fused widths firth_xtv_kernel) against tests/firth_reference.py: dense np.linalg.inv and explicit quadratic forms.

Bars (the project's):
  pass    scaled_err(A) <= 1e-9;  g*: nrel <= 1e-9 at a non-converged beta, |g - g_ref| <= 1e-9 sum_i |v_i| |x_ij|
          columnwise at the converged one (where g* cancels to about 0);  sum h, log det A, the deviance rel 1e-9;
          hat elementwise within 1e-9 of the reference and of Engine.influence's
  fits    conftest.check_fit with cond = cond(A) at the solution; the iteration count, at the epsilon the
          reference's trace of |delta|_1 is clearest of -- a factor 10 clear of every judged step (asserted);
          D* and log det A rel 1e-9; the same halvings

The reference's own error, measured on the CPU (tests/test_firth_reference.py asserts <= 1e-11 at 1300 x 20): fp64
against np.longdouble and against the rows in reverse order, A <= 2.8e-15, g* <= 1.0e-15, sum h <= 3.6e-16, hat <=
4.2e-17.  So the 1e-9 bars keep > 1e5 of margin from the reference alone.
"""
import numpy as np
import pytest

import firth_reference as F
from conftest import check_fit, nrel, rel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, _lib as L
from test_gpu_fe import SWEEP_P, sweep_n

pytestmark = pytest.mark.gpu

SEED = 2
CLEAR = 10.0  # the factor every judged step of a fit's reference trace stays clear of its epsilon


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


_cases = {}


def case(fam, lnk, n, p, seed=SEED):
    """The data of one case and its kwargs for the reference, made once per module."""
    key = (fam, lnk, n, p, seed)
    if key not in _cases:
        c = F.make_case(fam, lnk, n, p, seed)
        _cases[key] = (c, dict(m=c["m"], off=c["off"], pw=c["pw"]))
    return _cases[key]


def load(e, c, kw):
    e.set_data(c["X"], c["y"], m=kw["m"], offset=kw["off"], prior=kw["pw"])


def check_pass(label, e, c, kw, fam, lnk, beta, converged=False, influence=True):
    """firth_pass at beta against the reference's A, g*, sum h, log det A, the deviance and hat."""
    ref = F.firth_pass(c["X"], c["y"], beta, fam, lnk, **kw)
    got = e.firth_pass(beta, fam, lnk, hat=True)
    errs = dict(A=scaled_err(got["A"], ref["A"]), sum_hat=rel(got["sum_hat"], ref["sum_hat"]),
                logdet=rel(got["logdet"], ref["logdet"]), dev=rel(got["deviance"], ref["deviance"]),
                hat=float(np.max(np.abs(got["hat"] - ref["hat"]))))
    if converged:
        errs["g"] = float(np.max(np.abs(got["g"] - ref["g"]) / ref["scale"]))
    else:
        errs["g"] = nrel(got["g"], ref["g"])
    if influence:
        errs["hat_infl"] = float(np.max(np.abs(got["hat"] - e.influence(beta, fam, lnk).hat)))
    worst = max(errs.values())
    print(f"\nMARGIN {label}: {1e-9 / max(worst, 1e-300):.3g} (" + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) +
          f"; max |g*| {np.max(np.abs(ref['g'])):.2e}, firth_ms {e.firth_ms():.3f})")
    assert np.array_equal(got["A"], got["A"].T)
    assert np.all(got["hat"][kw["pw"] == 0.0] == 0.0) if kw["pw"] is not None else True
    assert worst <= 1e-9, (label, errs)
    return ref


@pytest.mark.parametrize("p", SWEEP_P)
def test_firth_pass_at_a_non_converged_point(eng, p):
    """Every width class of the kernel (one to sixteen column blocks, p off a multiple of 16, the fused route and
    the two-kernel one); rows that are no multiple of the 64-row step; trials m, an offset, prior weights with zeros."""
    n = sweep_n(p)
    c, kw = case("binomial", "logit", n, p)
    load(eng, c, kw)
    check_pass(f"firth_pass {n}x{p}", eng, c, kw, "binomial", "logit", c["beta"] * 0.8)


@pytest.mark.parametrize("p", (5, 129, 256))
def test_firth_pass_at_the_converged_point(eng, p):
    """There g* cancels to about 0: judged against sum_i |v_i| |x_ij|."""
    n = sweep_n(p)
    c, kw = case("binomial", "logit", n, p)
    load(eng, c, kw)
    o = F.firth_fit(c["X"], c["y"], "binomial", "logit", epsilon=1e-12, **kw)
    assert o["converged"]
    ref = check_pass(f"firth_pass converged {n}x{p}", eng, c, kw, "binomial", "logit", o["coefs"], converged=True)
    assert np.max(np.abs(ref["g"]) / ref["scale"]) < 1e-9  # the point of the case: the sum cancels


@pytest.mark.parametrize("n,p", [(50, 5), (449, 17), (300_001, 5), (80_001, 129), (1291, 160), (1291, 161)])
def test_shapes_that_can_go_wrong(eng, n, p):
    """Fewer rows than one workgroup step; 64 k + 1 rows; workgroups that take more than one step, with the
    accumulators carried across the grid-stride loop (more than twice the rows one grid sweep covers on a 256-CU
    device at 4 and at 2 workgroups per CU); the last fused width (ten column blocks) and the first two-kernel one."""
    fam, lnk = ("poisson", "log") if n == 449 else ("binomial", "logit")
    c, kw = case(fam, lnk, n, p)
    load(eng, c, kw)
    check_pass(f"firth_pass {n}x{p}", eng, c, kw, fam, lnk, c["beta"] * 0.8, influence=n < 100_000)


def check_firth_fit(label, e, c, kw, fam, lnk):
    long = F.firth_fit(c["X"], c["y"], fam, lnk, epsilon=1e-13, maxit=30, **kw)
    eps = F.pick_epsilon(long["trace"])
    clear = F.clearance(long["trace"], eps)
    print(f"\nCLEARANCE {label}: {clear:.3g} at epsilon {eps:.3g}")
    assert clear >= CLEAR, (label, clear, long["trace"])
    o = F.firth_fit(c["X"], c["y"], fam, lnk, epsilon=eps, **kw)
    r = e.fit_glm_firth(fam, lnk, eps, 100)
    check_fit(label, r.fit, o, float(np.linalg.cond(o["A"])))
    perr = max(rel(r.pen_deviance, o["pen_deviance"]), rel(r.logdet, o["logdet"]))
    print(f"MARGIN {label} D*, logdet: {1e-9 / max(perr, 1e-300):.3g} (iter {o['iter']}, halvings {o['halvings']}, "
          f"sum h {r.sum_hat!r}, |g*|_inf {r.score_inf:.2e})")
    assert r.converged and o["converged"] and r.halvings == o["halvings"] and perr <= 1e-9, (label, perr)
    assert abs(r.sum_hat - c["X"].shape[1]) <= 1e-9 * c["X"].shape[1]
    return r, o


@pytest.mark.parametrize("fam,lnk", F.PAIRS)
def test_every_pair_fits(eng, fam, lnk):
    c, kw = case(fam, lnk, 2000, 8)
    load(eng, c, kw)
    check_firth_fit(f"firth {fam}/{lnk}", eng, c, kw, fam, lnk)


@pytest.mark.parametrize("n,p", [(4001, 65), (12_001, 256)])
def test_wide_logit_fits(eng, n, p):
    c, kw = case("binomial", "logit", n, p)
    load(eng, c, kw)
    check_firth_fit(f"firth logit {n}x{p}", eng, c, kw, "binomial", "logit")


def test_separated_logit(eng):
    """3 / 10 against 7 / 7 replicated to 1700 rows: the closed form pi = (S + 1/2) / (n + 1) per cell, where the
    ordinary fit diverges."""
    k = 100
    x = np.r_[np.zeros(10 * k), np.ones(7 * k)]
    y = np.r_[np.ones(3 * k), np.zeros(7 * k), np.ones(7 * k)]
    X = np.asfortranarray(np.c_[np.ones(17 * k), x])
    eng.set_data(X, y)
    r = eng.fit_glm_firth("binomial", "logit", 1e-10, 100)
    lg = lambda q: np.log(q / (1 - q))
    b0, b1 = lg((3 * k + 0.5) / (10 * k + 1)), lg((7 * k + 0.5) / (7 * k + 1))
    want = np.array([b0, b1 - b0])
    err = float(np.max(np.abs(r.fit.coefs - want)))
    print(f"\nMARGIN separated logit: {1e-9 / max(err, 1e-300):.3g} (coefs {r.fit.coefs}, iter {r.fit.iter})")
    assert r.converged and err <= 1e-9
    try:
        f = eng.fit_glm("binomial", "logit", max_iter=25)
        assert np.max(np.abs(f.coefs)) > 10.0 or f.iter >= 25, (f.coefs, f.iter)
    except L.MatrixSingularException:
        pass  # the weights of the separated rows underflowed: no ordinary fit either


@pytest.mark.parametrize("p", (5, 64, 256))
def test_two_passes_are_bitwise_equal(eng, p):
    c, kw = case("binomial", "logit", sweep_n(p), p)
    load(eng, c, kw)
    a = eng.firth_pass(c["beta"] * 0.8, hat=True)
    b = eng.firth_pass(c["beta"] * 0.8, hat=True)
    for k in ("A", "g", "hat"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["sum_hat"], a["logdet"], a["deviance"]) == (b["sum_hat"], b["logdet"], b["deviance"])


@pytest.mark.parametrize("p", (33, 256))
def test_group_handle_matches_the_single_handle(eng, p):
    n = sweep_n(p)
    c, kw = case("binomial", "logit", n, p)
    load(eng, c, kw)
    beta = c["beta"] * 0.8
    one = eng.firth_pass(beta, hat=True)
    f1 = eng.fit_glm_firth("binomial", "logit", 1e-8, 100)
    with Engine(devices=[0, 0]) as g:
        load(g, c, kw)
        two = g.firth_pass(beta, hat=True)
        f2 = g.fit_glm_firth("binomial", "logit", 1e-8, 100)
        assert g.firth_ms() > 0.0
    errs = dict(g=nrel(two["g"], one["g"]), A=scaled_err(two["A"], one["A"]),
                hat=float(np.max(np.abs(two["hat"] - one["hat"]))), coefs=rel(f2.fit.coefs, f1.fit.coefs),
                stderr=rel(f2.fit.stderr, f1.fit.stderr), pen=rel(f2.pen_deviance, f1.pen_deviance))
    print(f"\nMARGIN group {n}x{p}: {1e-9 / max(max(errs.values()), 1e-300):.3g} ({errs})")
    assert max(errs.values()) <= 1e-9 and f2.fit.iter == f1.fit.iter and f2.converged and f2.halvings == f1.halvings


def test_wrapper_round_trip(eng):
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    c, kw = case("binomial", "logit", 2000, 8)
    names = ["(Intercept)"] + [f"x{j}" for j in range(1, 8)]
    x = Frame({nm: c["X"][:, j].copy() for j, nm in enumerate(names)})
    y, m = Frame({"y": c["y"]}), Frame({"m": kw["m"]})
    off, pw = Frame({"off": kw["off"]}), Frame({"w": kw["pw"]})
    obj = GLM.fit_firth(y, x, "binomial", "logit", offset=off, m=m, prior=pw, epsilon=1e-8)
    o = F.firth_fit(c["X"], c["y"], "binomial", "logit", epsilon=1e-8, **kw)
    assert obj.converged and obj.aic is None and obj.halvings == o["halvings"] and obj.iter == o["iter"]
    assert rel(np.asarray(obj.coefs).reshape(-1), o["coefs"]) <= 1e-9 and rel(obj.stdErr, o["stderr"]) <= 1e-9
    assert rel(obj.pen_deviance, o["pen_deviance"]) <= 1e-9 and rel(obj.logdet, o["logdet"]) <= 1e-9
    text = GLM.summary_string(obj)
    assert "Firth's penalized likelihood" in text and "AIC:" not in text
    new = Frame({nm: c["X"][:5, j].copy() for j, nm in enumerate(names)})
    eta = c["X"][:5] @ o["coefs"]
    assert rel(obj.predict(new, type="link")["value"], eta) <= 1e-9
    V = GLM.vcov(obj, y, x, offset=off, m=m, prior=pw)
    assert rel(np.sqrt(np.diag(V)), o["stderr"]) <= 1e-9
    tab = GLM.coeftest(obj, y, x, offset=off, m=m, prior=pw, type="HC0")
    V0 = GLM.vcov(obj, y, x, offset=off, m=m, prior=pw, type="HC0")
    assert rel(tab["se"], np.sqrt(np.diag(V0))) <= 1e-12
    assert rel(tab["stat"], o["coefs"] / np.sqrt(np.diag(V0))) <= 1e-8
    inf = GLM.influence(obj, y, x, offset=off, m=m, prior=pw)
    assert abs(inf.sum_hat - 8) <= 1e-9 * 8
