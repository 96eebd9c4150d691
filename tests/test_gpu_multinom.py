"""Multinomial logit fits on the GPU (sglm_fit_multinom, sglm_multinom_pass: multinom.hip's multinom_rows_kernel,
multinom_xtr_kernel past the fused shapes, multinom_weight_kernel and the Gram pass per block pair of the Hessian)
against tests/multinom_reference.py.

Bars (the project's):
  pass    scaled_err(H) <= 1e-9;  g: nrel <= 1e-9 at a non-converged B (0.8 B_true), |g - g_ref| <= 1e-9 sum_i |R_ij|
          |x_ic| columnwise at the converged one (where g cancels to about 0);  deviance, sum pw, the null deviance
          and the class counts rel 1e-9;  P elementwise within 1e-9
  fits    conftest.check_fit with cond = cond(H) at the solution; the iteration count and the halvings, at the
          epsilon the reference's trace is clearest of -- a factor 10 clear of every judged step (asserted)
  rows    P against the np.longdouble reference within the bar derived below (prob_bar), never a measured one

The reference's own error, measured on the CPU (tests/test_multinom_reference.py asserts <= 1e-11 at 1300 x 20):
H <= 5.2e-15, g <= 4.1e-15, deviance <= 1.1e-16, P <= 1.2e-16: the 1e-9 bars keep > 1e5 of margin from it.

The fused / two-kernel threshold of the build (multinom.hip MN_FUSED_MAX = 21: fused while P16 (KM + 1) <= 21, KM the
bucket 1, 2, 3, 4, 7, 15 holding K - 1): K = 3 fused to P16 = 7 (p = 112), two kernels from p = 113; K = 2 fused to
p = 160; K = 16 fused at p <= 16 only.
"""
import numpy as np
import pytest

import multinom_reference as M
from conftest import check_fit, nrel, rel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, Multinom, _lib as L
from sparkglm_amd.frame import Frame
from test_gpu_fe import SWEEP_P, sweep_n

pytestmark = pytest.mark.gpu

SEED = 2
CLEAR = 10.0  # the factor every judged step of a fit's reference trace stays clear of its epsilon
U = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


_cases = {}


def case(n, p, K, seed=SEED):
    key = (n, p, K, seed)
    if key not in _cases:
        _cases[key] = M.make_case(n, p, K, seed)
    return _cases[key]


def load(e, c):
    e.set_data(c["X"], c["y"], prior=c["pw"])


def check_pass(label, e, c, K, B, converged=False):
    """multinom_pass at B against the reference's H, g, scalars and P."""
    ref = M.multinom_pass(c["X"], c["y"], B, c["pw"])
    got = e.multinom_pass(B, K, prob=True)
    errs = dict(H=scaled_err(got["H"], ref["H"]), dev=rel(got["deviance"], ref["deviance"]),
                sum_w=rel(got["sum_w"], ref["sum_w"]), null=rel(got["null_deviance"], ref["null_deviance"]),
                P=float(np.max(np.abs(got["prob"] - ref["P"]))))
    if converged:
        errs["g"] = float(np.max(np.abs(got["g"] - ref["g"]) / ref["scale"]))
    else:
        errs["g"] = nrel(got["g"], ref["g"])
    worst = max(errs.values())
    ms = e.multinom_ms()
    print(f"\nMARGIN {label}: {1e-9 / max(worst, 1e-300):.3g} (" + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) +
          f"; max |g| {np.max(np.abs(ref['g'])):.2e}, rows {ms[0]:.3f} xtr {ms[1]:.3f} weight {ms[2]:.3f} gram "
          f"{ms[3]:.3f} ms)")
    assert np.array_equal(got["H"], got["H"].T)
    assert worst <= 1e-9, (label, errs)
    return ref, got


@pytest.mark.parametrize("p", SWEEP_P)
def test_width_sweep(eng, p):
    """Every width class of the row kernel at K = 3 (one to sixteen column blocks, p off a multiple of 16, the
    fused route and from p = 113 the two-kernel one); rows that are no multiple of the 64-row step; prior weights
    with zeros."""
    n = sweep_n(p)
    c = case(n, p, 3)
    load(eng, c)
    check_pass(f"multinom_pass {n}x{p} K=3", eng, c, 3, 0.8 * c["B"])


@pytest.mark.parametrize("p", (5, 17))
@pytest.mark.parametrize("K", (2, 3, 4, 9, 16))
def test_class_sweep(eng, K, p):
    """Every class bucket of the fused form (1, 2, 3, 4, 7, 15), and at p = 17 the two-kernel route from K = 9."""
    c = case(1501, p, K)
    load(eng, c)
    check_pass(f"multinom_pass 1501x{p} K={K}", eng, c, K, 0.8 * c["B"])


@pytest.mark.parametrize("p,K", [(112, 3), (113, 3), (160, 2), (161, 2), (16, 16), (32, 8), (33, 8), (80, 4), (81, 4),
                                 (64, 5), (65, 5)])
def test_threshold_shapes(eng, p, K):
    """The last fused and the first two-kernel width of every class bucket."""
    c = case(1291, p, K)
    load(eng, c)
    _, got = check_pass(f"multinom_pass 1291x{p} K={K}", eng, c, K, 0.8 * c["B"])
    P16, KM = (p + 15) // 16, next(b for b in (1, 2, 3, 4, 7, 15) if K - 1 <= b)
    assert (eng.multinom_ms()[1] == 0.0) == (P16 * (KM + 1) <= 21)  # X'R ran exactly past the threshold


@pytest.mark.parametrize("n,p,K", [(50, 5, 3), (449, 17, 4), (300_001, 5, 3), (80_001, 129, 3), (1291, 256, 5)])
def test_shapes_that_can_go_wrong(eng, n, p, K):
    """Fewer rows than one workgroup step; 64 k + 1 rows; workgroups that take more than two steps, with the
    accumulators carried across the grid-stride loop (more than twice the rows one grid sweep covers on a 256-CU
    device at two workgroups per CU: 9 and 2.4 sweeps), fused and two-kernel; the largest q = 1024."""
    c = case(n, p, K)
    load(eng, c)
    check_pass(f"multinom_pass {n}x{p} K={K}", eng, c, K, 0.8 * c["B"])


@pytest.mark.parametrize("p,K", [(5, 3), (129, 3)])
def test_pass_at_the_converged_point(eng, p, K):
    """There g cancels to about 0: judged against sum_i |R_ij| |x_ic|."""
    n = sweep_n(p)
    c = case(n, p, K)
    load(eng, c)
    o = M.multinom_fit(c["X"], c["y"], K, c["pw"], epsilon=1e-13)
    assert o["converged"]
    ref, _ = check_pass(f"multinom_pass converged {n}x{p}", eng, c, K, o["B"], converged=True)
    assert np.max(np.abs(ref["g"]) / ref["scale"]) < 1e-9  # the point of the case: the sum cancels


# ---- row by row ----
def prob_bar(P, a):
    """The bar of pi_j in units of 2^-53 pi_j, by first-order propagation of the stated errors of what the kernel
    calls (one correctly rounded operation 1 unit; a libm primitive good to 1 ulp 2 units; errors of shared
    operands added without using their correlation), P and a = eta - mx from the long double reference:
      a_j = eta_j - mx 1 unit of |a_j|, which reaches exp as |a_j| units;  E_j = exp(a_j): 2 + |a_j|
      S = E_0 + ...: K - 1 additions of at most 1 unit of S each, and the terms' own: sum_l pi_l (2 + |a_l|)
      pi_j = E_j / S: 1
    -- 3 + |a_j| + (K - 1) + sum_l pi_l (2 + |a_l|).  (eta itself is exact in the rows of this test.)  Where E_j is
    subnormal or 0 its error is at most one subnormal step, 2^-1074 (S >= 1): the absolute floor."""
    K = P.shape[1]
    a = np.abs(a)
    return 3.0 + a + (K - 1) + np.sum(np.where(P > 0, P * (2.0 + a), 0.0), axis=1, keepdims=True)


def test_row_by_row(eng):
    """prob against the long double reference row by row.  Every row has a single 1 in its design, so eta_j is the
    coefficient itself, exactly: moderate values, +-30, +-700, beyond exp's overflow (800) and a row whose own
    class's pi underflows (eta_y - mx = -1500); rows of weight 0 (their y is not looked at: a code out of range)."""
    K = 4
    etas = np.array([[0.0, 0.0, 0.0], [0.3, -1.2, 2.5], [30.0, -30.0, 1.0], [-30.0, -30.0, -30.0],
                     [700.0, -700.0, 0.5], [-700.0, -700.0, -700.0], [800.0, 2.0, -800.0], [-800.0, 799.0, 800.0],
                     [700.0, 699.0, 698.5], [-1e-3, 1e-3, 1e-9], [745.0, -745.2, 10.0], [36.7, -36.7, 0.1]])
    p = len(etas)
    reps = 7  # 84 rows: more than one workgroup step
    idx = np.tile(np.arange(p), reps)
    n = len(idx)
    X = np.zeros((n, p), order="F")
    X[np.arange(n), idx] = 1.0
    B = etas.copy()  # [p, K - 1]
    y = (np.arange(n) % K).astype(np.float64)
    y[6] = 3.0   # eta = (0, 800, 2, -800): the row's own class underflows, log pi_y = -1600
    pw = 1.0 + (np.arange(n) % 3).astype(np.float64)
    dead = np.arange(n) % 11 == 5
    pw[dead] = 0.0
    y[dead] = 99.0
    eng.set_data(X, y, prior=pw)
    got = eng.multinom_pass(B, K, prob=True, hessian=False)
    ld = M.rows(X, y, B, pw, dtype=np.longdouble)
    Pl = ld["P"]
    e = np.concatenate([np.zeros((n, 1), dtype=np.longdouble), ld["eta"]], axis=1)
    a = e - np.max(e, axis=1, keepdims=True)
    bar = np.asarray(prob_bar(Pl, a) * U * Pl, dtype=np.float64) + 2.0 ** -1074
    err = np.abs(got["prob"].astype(np.longdouble) - Pl).astype(np.float64)
    print(f"\nMARGIN row by row P: {float(np.min(np.where(err > 0, bar / np.where(err > 0, err, 1), np.inf))):.3g} "
          f"(worst bar {float(np.max(prob_bar(Pl, a))):.0f} units)")
    assert np.all(np.isfinite(got["prob"])) and np.isfinite(got["deviance"])
    assert np.all(err <= bar), np.argwhere(err > bar)
    assert np.max(np.abs(np.sum(got["prob"], axis=1) - 1.0)) <= K * 2.0 ** -52
    live = pw > 0
    dev = float(-2 * np.sum(np.where(live, ld["pw"] * ld["logpy"], 0)))
    assert rel(got["deviance"], dev) <= 1e-9 and got["deviance"] > 3000.0
    # rows of weight 0 give exact zeros in R: the score is the live rows' alone (the reference's R has the zeros)
    ref = M.multinom_pass(X, y, B, pw)
    assert np.all(np.isfinite(got["g"])) and np.max(np.abs(got["g"] - ref["g"]) / np.maximum(ref["scale"], 1e-300)) <= 1e-9


def test_rows_of_weight_zero_contribute_exact_zeros(eng):
    """Their design entries are 1e150 and their y is out of range: anything but an exact 0 in R would show in g."""
    c = case(449, 17, 4)
    X, y, pw = c["X"].copy(order="F"), c["y"].copy(), c["pw"].copy()
    dead = pw == 0
    assert np.sum(dead) > 50
    X[dead, 1:] = 1e150
    y[dead] = 99.0
    eng.set_data(X, y, prior=pw)
    got = eng.multinom_pass(0.8 * c["B"], 4, hessian=False, score=True)
    eng.set_data(np.asfortranarray(c["X"][~dead]), c["y"][~dead], prior=c["pw"][~dead])
    live = eng.multinom_pass(0.8 * c["B"], 4, hessian=False, score=True)
    ref = M.multinom_pass(c["X"], c["y"], 0.8 * c["B"], c["pw"])
    assert nrel(got["g"], ref["g"]) <= 1e-9 and nrel(live["g"], ref["g"]) <= 1e-9
    assert rel(got["deviance"], ref["deviance"]) <= 1e-9 and got["sum_w"] == ref["sum_w"]


# ---- fits ----
def check_multinom_fit(label, e, c, K):
    long = M.multinom_fit(c["X"], c["y"], K, c["pw"], epsilon=1e-15, max_iter=12)
    eps = M.pick_epsilon(long["trace"])
    clear = M.clearance(long["trace"], eps)
    print(f"\nCLEARANCE {label}: {clear:.3g} at epsilon {eps:.3g} (trace {long['trace']})")
    assert clear >= CLEAR, (label, clear, long["trace"])
    o = M.multinom_fit(c["X"], c["y"], K, c["pw"], epsilon=eps)
    r = e.fit_multinom(K, eps, 100)
    cond = float(np.linalg.cond(o["H"]))
    check_fit(label, r, o, cond)
    serr = max(rel(r.aic, o["aic"]), rel(r.class_weight, o["counts"]), scaled_err(r.cov, o["cov"]))
    print(f"MARGIN {label} aic, counts, cov: {1e-9 / max(serr, 1e-300):.3g} (iter {o['iter']}, halvings "
          f"{o['halvings']}, cond {cond:.2e}, |g|_inf {r.score_inf:.2e})")
    assert r.converged and o["converged"] and r.halvings == o["halvings"] and serr <= 1e-9, (label, serr)
    assert 3 <= o["iter"] <= 7 and cond <= 1e3
    return r, o


@pytest.mark.parametrize("n,p,K", [(2000, 8, 3), (4001, 33, 4), (12_001, 64, 5), (20_001, 128, 3), (6001, 17, 16)])
def test_fits(eng, n, p, K):
    c = case(n, p, K)
    load(eng, c)
    check_multinom_fit(f"multinom fit {n}x{p} K={K}", eng, c, K)


def test_k2_is_the_binomial_logit_fit(eng):
    c = case(4001, 33, 2)
    load(eng, c)
    r = eng.fit_multinom(2, 1e-12, 100)
    f = eng.fit_glm("binomial", "logit", tol=1e-10)
    errs = dict(coefs=rel(r.coefs[0], f.coefs), stderr=rel(r.stderr[0], f.stderr), dev=rel(r.deviance, f.deviance))
    one = eng.multinom_pass(r.coefs.T, 2)
    G, _, _ = eng.irls_pass(np.ascontiguousarray(r.coefs[0]), family="binomial", link="logit")
    errs["H"] = scaled_err(one["H"], G)
    print(f"\nMARGIN K = 2 against fit_glm: {1e-9 / max(max(errs.values()), 1e-300):.3g} ({errs})")
    assert r.converged and max(errs.values()) <= 1e-9, errs


@pytest.mark.parametrize("p", (5, 64, 256))
def test_two_passes_are_bitwise_equal(eng, p):
    c = case(sweep_n(p), p, 3)
    load(eng, c)
    a = eng.multinom_pass(0.8 * c["B"], 3, prob=True)
    b = eng.multinom_pass(0.8 * c["B"], 3, prob=True)
    for k in ("H", "g", "prob"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["deviance"], a["sum_w"], a["null_deviance"]) == (b["deviance"], b["sum_w"], b["null_deviance"])
    d = eng.multinom_pass(0.8 * c["B"], 3, hessian=False)
    assert rel(d["deviance"], a["deviance"]) <= 1e-14  # the deviance-only evaluation


@pytest.mark.parametrize("p", (33, 256))
def test_group_handle_matches_the_single_handle(eng, p):
    n = sweep_n(p)
    c = case(n, p, 3)
    load(eng, c)
    B = 0.8 * c["B"]
    one = eng.multinom_pass(B, 3, prob=True)
    f1 = eng.fit_multinom(3, 1e-8, 100)
    with Engine(devices=[0, 0]) as g:
        load(g, c)
        two = g.multinom_pass(B, 3, prob=True)
        f2 = g.fit_multinom(3, 1e-8, 100)
        assert g.multinom_ms()[0] > 0.0
    errs = dict(g=nrel(two["g"], one["g"]), H=scaled_err(two["H"], one["H"]), dev=rel(two["deviance"], one["deviance"]),
                P=float(np.max(np.abs(two["prob"] - one["prob"]))), coefs=rel(f2.coefs, f1.coefs),
                stderr=rel(f2.stderr, f1.stderr), fdev=rel(f2.deviance, f1.deviance))
    print(f"\nMARGIN group {n}x{p}: {1e-9 / max(max(errs.values()), 1e-300):.3g} ({errs})")
    assert max(errs.values()) <= 1e-9 and f2.iter == f1.iter and f2.converged and f2.halvings == f1.halvings


def test_errors(eng):
    c = case(449, 17, 4)
    B = 0.8 * c["B"]
    y = c["y"].copy()
    live = np.nonzero(c["pw"] > 0)[0]
    y[live[3]] = 1.5
    eng.set_data(c["X"], y, prior=c["pw"])
    for call in (lambda: eng.multinom_pass(B, 4), lambda: eng.fit_multinom(4)):
        with pytest.raises(L.IllegalArgumentException, match="integer class code"):
            call()
    y = c["y"].copy()
    y[live[5]] = 4.0
    eng.set_data(c["X"], y, prior=c["pw"])
    with pytest.raises(L.IllegalArgumentException, match="integer class code"):
        eng.multinom_pass(B, 4)
    eng.set_data(c["X"], np.where(c["y"] == 2.0, 1.0, c["y"]), prior=c["pw"])
    with pytest.raises(L.IllegalArgumentException, match="class 2 has none"):
        eng.fit_multinom(4)
    eng.set_data(c["X"], c["y"], prior=c["pw"], offset=np.zeros(449))
    with pytest.raises(L.IllegalArgumentException, match="no trials m and no offset"):
        eng.multinom_pass(B, 4)
    eng.set_data(c["X"], c["y"], prior=c["pw"], m=np.ones(449))
    with pytest.raises(L.IllegalArgumentException, match="no trials m and no offset"):
        eng.fit_multinom(4)
    c = case(300, 129, 9)
    load(eng, c)
    with pytest.raises(L.IllegalArgumentException, match=r"\(n_classes - 1\) \* p <= 1024 \(got 1032\)"):
        eng.multinom_pass(np.zeros(1032), 9)


def test_wrapper_round_trip(eng):
    c = case(2000, 8, 3)
    names = ["(Intercept)"] + [f"x{j}" for j in range(1, 8)]
    x = Frame({nm: c["X"][:, j].copy() for j, nm in enumerate(names)})
    labels = np.array(["bird", "ant", "cat"])[c["y"].astype(int)]  # sorted: ant < bird < cat
    code = {0: 1, 1: 0, 2: 2}  # class code of make_case -> the level's position
    yc = np.array([code[int(v)] for v in c["y"]], dtype=np.float64)
    obj = Multinom.fit(Frame({"animal": labels}), x, prior=Frame({"w": c["pw"]}), epsilon=1e-8)
    o = M.multinom_fit(c["X"], yc, 3, c["pw"], epsilon=1e-8)
    assert list(obj.levels) == ["ant", "bird", "cat"] and obj.converged and obj.iter == o["iter"]
    assert rel(obj.coefs, o["coefs"]) <= 1e-9 and rel(obj.stdErr, o["stderr"]) <= 1e-9
    assert rel([obj.deviance, obj.null_deviance, obj.aic, obj.loglik],
               [o["deviance"], o["null_deviance"], o["aic"], o["loglik"]]) <= 1e-9
    assert rel(obj.z, o["coefs"] / o["stderr"]) <= 1e-8 and np.all((obj.pvalue >= 0) & (obj.pvalue <= 1))
    new = Frame({nm: c["X"][:7, j].copy() for j, nm in enumerate(names)})
    want = M.rows(c["X"][:7], np.zeros(7), o["B"])["P"]
    assert np.max(np.abs(obj.predict(new) - want)) <= 1e-9
    assert rel(obj.predict(new, type="link"), c["X"][:7] @ o["B"]) <= 1e-9
    assert list(obj.predict(new, type="class")) == list(np.array(["ant", "bird", "cat"])[np.argmax(want, axis=1)])
    text = Multinom.summary_string(obj)
    assert "Baseline: ant" in text and "bird:" in text and "cat:" in text and "Residual Deviance" in text
    assert obj.table("coefs").columns == ["level"] + names
