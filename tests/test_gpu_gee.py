"""GEE fits with an exchangeable working correlation on the GPU (sglm_fit_glm_gee, sglm_gee_pass, sglm_vcov_gee:
the kernels of gee.hip, the segment-sum and combine kernels of cluster.hip, a Gram pass over the group sums)
against tests/gee_reference.py: explicit dense blocks R_g and np.linalg.solve per cluster, never the closed form
c_g the engine downdates with.

Bars (the project's):
  pass    scaled_err(A) <= 1e-9;  b, s, t, n, E, Q: nrel <= 1e-9;  each moment, rho and the pass's scalars rel <= 1e-9
  fits    conftest.check_fit with cond = ||X'WX||_2 ||inv(A)||_2 (the downdate loses that factor, not cond(A));
          dev_trace elementwise 1e-9; the iteration count, at the tol the reference's trace is clearest of:
          a factor 10 clear of every judged step, except the recorded cases of WEAK_CLEARANCE;
          rho and phi at the returned coefficients rel 1e-9
  V       scaled_err <= test_gpu_fe.v_bar(cond) = 2 max(1e-9, K_BOUND cond eps)

The reference's own error, measured on the CPU (tests/test_gee_reference.py asserts <= 1e-11 at 1300 x 20 for
every id pattern): fp64 against np.longdouble and against the rows in reverse order, A <= 1.5e-15, b <= 7.0e-16,
the moments <= 7.9e-16, s / t / E / Q <= 1.2e-15, V <= 7.1e-15.  So the 1e-9 bars keep > 1e5 of margin from the
reference alone.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import fe_reference as FR
import gee_reference as GR
import links_reference as LR
import np_reference as R
from conftest import check_fit, nrel, rel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D
from test_gpu_fe import FAMILY_CASES, SWEEP_P, T, sweep_n, v_bar

pytestmark = pytest.mark.gpu

SEED = 2


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


_cases = {}


def case(fam, lnk, n, p, pattern, seed=SEED):
    """The data of one case and its kwargs for the reference, made once per module."""
    key = (fam, lnk, n, p, pattern, seed)
    if key not in _cases:
        ids, G = FR.make_ids(pattern, n, T)
        c = GR.make_case(fam, lnk, n, p, ids, G, seed)
        kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
        if fam == "negbin":
            kw["theta"] = 2.0
        _cases[key] = (c, ids, G, kw)
    return _cases[key]


def load(e, c, ids, G, kw):
    if "theta" in kw:
        e.set_theta(kw["theta"])
    e.set_data(c["X"], c["y"], m=kw["m"], offset=kw["off"], prior=kw["pw"])
    e.set_clusters(ids, G)


def downdate_cond(ref):
    return float(np.linalg.norm(ref["XtWX"], 2) * np.linalg.norm(np.linalg.inv(ref["A"]), 2))


def negative_rho(ids, pw=None):
    """A negative rho inside the valid range 1 - rho + n_max rho > 0 of the case's largest cluster."""
    n_max = int(np.bincount(ids, weights=None if pw is None else (pw > 0).astype(float)).max())
    return -0.5 / (n_max - 1)


def check_pass(label, e, c, ids, G, kw, fam, lnk, beta, rho=None, corstr="exchangeable", mode=None):
    """gee_pass at beta against the reference's A, b, the group sums, the moments, rho and the pass's scalars."""
    if beta is None:
        mu0 = float(np.sum(c["y"])) / len(c["y"])
        ref = GR.gee_pass(c["X"], c["y"], None, ids, G, fam, lnk, rho=rho, corstr=corstr, mode=mode or 1, mu0=mu0, **kw)
    else:
        ref = GR.gee_pass(c["X"], c["y"], beta, ids, G, fam, lnk, rho=rho, corstr=corstr, **kw)
    got = e.gee_pass(beta, fam, lnk, corstr=corstr, rho=rho, init="multiple" if mode == 2 else "single")
    errs = dict(A=scaled_err(got["A"], ref["A"]), b=nrel(got["b"], ref["b"]))
    for k in ("s", "t", "n", "E", "Q"):
        errs[k] = nrel(got[k], ref[k])
    for k, name in enumerate(("sumE2", "sumQ", "pairs", "N", "n_max")):  # separately: E^2 - Q cancels in rho
        errs[name] = rel(got["moments"][k], ref["moments"][k])
    if ref["rho"] == 0.0:
        assert got["rho"] == 0.0, (label, got["rho"])
    else:
        errs["rho"] = rel(got["rho"], ref["rho"])
    if beta is not None and fam == "poisson" and lnk == "log":
        mu = np.exp(c["X"] @ beta + kw["off"])
        dev = R.deviance("poisson", c["y"], mu, np.ones(len(mu)), kw["pw"], 1)
        errs["dev"] = abs(2.0 * got["scalars"][L.S_DEV] - dev) / abs(dev)
        errs["sumw"] = abs(got["scalars"][L.S_SUMW] - kw["pw"].sum()) / kw["pw"].sum()
    worst = max(errs.values())
    print(f"\nMARGIN {label}: {1e-9 / max(worst, 1e-300):.3g} (" + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) +
          f"; rho {ref['rho']:.4f}, cond {downdate_cond(ref):.2e}, G {G})")
    assert np.array_equal(got["A"], got["A"].T)
    assert worst <= 1e-9, (label, errs)
    return ref


@pytest.mark.parametrize("p", SWEEP_P)
def test_gee_pass_at_a_non_converged_point(eng, p):
    """Every width of the segment sums and of the Gram pass over the group rows; rows that are no multiple of 32
    or of the tile; estimated rho, a fixed one and a negative one (the sign path); the initial mode."""
    n = sweep_n(p)
    for pat in ("sorted", "shuffled") + (("interleaved", "two_level") if p == 65 else ()):
        c, ids, G, kw = case("poisson", "log", n, p, pat)
        load(eng, c, ids, G, kw)
        beta = c["beta"] * 0.8
        for rho in (None, 0.3, negative_rho(ids)):
            check_pass(f"gee_pass {n}x{p} {pat} rho={rho}", eng, c, ids, G, kw, "poisson", "log", beta, rho=rho)
    ref = check_pass(f"gee_pass init {n}x{p}", eng, c, ids, G, kw, "poisson", "log", None)
    assert ref["rho"] == 0.0


def pick_tol(trace):
    """The tol in [1e-7, 1e-3] that the reference's long trace is clearest of: the geometric mean of two
    consecutive steps, where links_reference.clearance is largest."""
    d = np.abs(np.diff(trace))
    cands = [float(np.sqrt(d[k] * d[k + 1])) for k in range(len(d) - 1) if d[k + 1] > 0.0]
    cands = [t for t in cands if 1e-7 <= t <= 1e-3]
    return max(cands, key=lambda t: LR.clearance(trace, t))


# The fits whose reference trace has no tol in [1e-7, 1e-3] a factor CLEAR_FULL = 10 clear of every step it
# judges, with the clearance their clearest tol reaches (measured on the CPU at SEED = 2).  With rho re-estimated at
# every step the iteration converges linearly -- the steps of these cases shrink 7x to 40x per iteration, so the best
# clearance is about sqrt of that.  They run at links_reference's floor CLEAR_MIN = 1.5: |step - tol| is then
# >= tol / 3 >= 3e-8, against ~1e-13 * deviance <= 1e-9 of summation-order difference between two correct
# implementations.  Every other fit (binomial / logit 27, binomial / probit 52, gamma / inverse 15, gaussian /
# identity 43, poisson 1286 x 65 17, the fixed rho 12.4) must keep CLEAR_FULL.  A case of this list that reaches
# CLEAR_FULL after a change to the reference or the cases fails too: take it off the list.
WEAK_CLEARANCE = {
    "poisson 1271x1": 3.29, "poisson 1331x5": 2.88, "poisson 1286x16": 2.58, "poisson 1301x17": 5.05,
    "poisson 1331x33": 3.81, "poisson 1271x64": 7.7, "poisson 1301x129": 8.7, "poisson 1316x256": 4.11,
    "binomial/cloglog": 7.94, "gamma/log": 9.23, "poisson/sqrt": 4.46, "negbin/log": 4.23,
    "negative fixed rho": 8.31, "big interleaved": 4.28, "big sorted": 5.99,
    "iris gaussian/identity": 3.53, "iris gamma/log": 1.93,
}


def clear_tol(label, trace):
    """The tol the reference's long trace is clearest of, with the floor of its case asserted."""
    tol = pick_tol(trace)
    clear = LR.clearance(trace, tol)
    print(f"\nCLEARANCE {label}: {clear:.3g} at tol {tol:.3g}")
    if label in WEAK_CLEARANCE:
        assert LR.CLEAR_MIN <= clear < LR.CLEAR_FULL, (label, clear, np.abs(np.diff(trace)))
    else:
        assert clear >= LR.CLEAR_FULL, (label, clear, np.abs(np.diff(trace)))
    return tol


def check_gee_fit(label, e, c, ids, G, kw, fam, lnk, rho=None, corstr="exchangeable"):
    """The fit at the tol its reference trace is clearest of (clear_tol): a factor 10 clear of every judged step,
    except the cases of WEAK_CLEARANCE."""
    long = GR.gee_fit(c["X"], c["y"], ids, G, fam, lnk, rho=rho, corstr=corstr, tol=1e-11, max_iter=30, **kw)
    tol = clear_tol(label, long["dev_trace"])
    o = GR.gee_fit(c["X"], c["y"], ids, G, fam, lnk, rho=rho, corstr=corstr, tol=tol, **kw)
    r = e.fit_glm_gee(fam, lnk, corstr=corstr, rho=rho, tol=tol)
    cond = downdate_cond(o)
    check_fit(label, r.fit, o, cond)
    terr = rel(r.fit.dev_trace, o["dev_trace"])
    perr = max(rel(r.rho, o["rho"]) if o["rho"] != 0.0 else abs(r.rho), rel(r.phi, o["phi"]))
    print(f"MARGIN {label} trace: {1e-9 / max(terr, 1e-300):.3g}; rho, phi: {1e-9 / max(perr, 1e-300):.3g} "
          f"(rho {o['rho']:.4f}, phi {o['phi']:.4f}, iter {o['iter']})")
    assert len(r.fit.dev_trace) == o["iter"] + 1 and terr <= 1e-9, (label, terr)
    assert perr <= 1e-9, (label, r.rho, o["rho"], r.phi, o["phi"])
    pw = kw["pw"]
    assert r.N == (len(c["y"]) if pw is None else int(np.sum(pw > 0))) and r.G_eff == G
    return r, o, cond, tol


@pytest.mark.parametrize("p", SWEEP_P)
def test_poisson_fits_match_the_reference(eng, p):
    n = sweep_n(p)
    c, ids, G, kw = case("poisson", "log", n, p, "sorted")
    load(eng, c, ids, G, kw)
    check_gee_fit(f"poisson {n}x{p}", eng, c, ids, G, kw, "poisson", "log")


@pytest.mark.parametrize("fam,lnk", [fc[:2] for fc in FAMILY_CASES])
def test_every_family_matches_the_reference(eng, fam, lnk):
    """3001 x 20, groups of 5-row runs: binomial with trials m, poisson / negbin (theta = 2) with offset and prior."""
    c, ids, G, kw = case(fam, lnk, 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    check_gee_fit(f"{fam}/{lnk}", eng, c, ids, G, kw, fam, lnk)


def test_fixed_rho_fit_and_the_multiple_init_mode(eng):
    """A fixed rho (Stata's corr(fixed)): the fit is Newton's again.  The initial mode of several partitions."""
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    r, _, _, _ = check_gee_fit("fixed rho", eng, c, ids, G, kw, "poisson", "log", rho=0.25)
    assert r.rho == 0.25
    r, _, _, _ = check_gee_fit("negative fixed rho", eng, c, ids, G, kw, "poisson", "log", rho=negative_rho(ids))
    ref = check_pass("gee_pass init multiple", eng, c, ids, G, kw, "poisson", "log", None, mode=2)
    assert ref["rho"] == 0.0


@pytest.mark.parametrize("fam,lnk", (("poisson", "log"), ("binomial", "logit")))
def test_independence_is_fit_glm_bitwise_and_its_robust_covariance_is_vcov_cluster(eng, fam, lnk):
    """(binomial / logit without trials: fit_glm's narrow pass carries its statistics in the pass, the GEE fit's
    passes store eta instead -- A, b and the deviance must not notice)"""
    c, ids, G, kw = case(fam, lnk, 3001, 20, "two_level")
    if fam == "binomial":
        kw = dict(kw, m=None)
        c = dict(c, y=(2.0 * c["y"] > c["m"]).astype(np.float64))
    load(eng, c, ids, G, kw)
    plain = eng.fit_glm(fam, lnk)
    r = eng.fit_glm_gee(fam, lnk, corstr="independence")
    assert np.array_equal(r.fit.coefs, plain.coefs) and np.array_equal(r.fit.dev_trace, plain.dev_trace)
    assert r.fit.iter == plain.iter and r.rho == 0.0
    got = eng.gee_pass(plain.coefs, fam, lnk, corstr="independence")
    G0, b0, _ = eng.irls_pass(plain.coefs, family=fam, link=lnk)
    assert np.array_equal(got["A"], G0) and np.array_equal(got["b"], np.asarray(b0).reshape(-1))
    for ca in (False, True):
        V = eng.vcov_gee(plain.coefs, 0.0, fam, lnk, corstr="independence", cadjust=ca)
        Vc = eng.vcov_cluster(plain.coefs, fam, lnk, type="HC0", cadjust=ca)
        e = scaled_err(V, Vc)
        print(f"\nMARGIN independence {fam} vs vcov_cluster cadjust={ca}: {1e-12 / max(e, 1e-300):.3g} (err {e:.2e})")
        assert e <= 1e-12


def test_gaussian_identity_with_fixed_rho_is_dense_gls(eng):
    c, ids, G, kw = case("gaussian", "identity", sweep_n(20), 20, "sorted")
    load(eng, c, ids, G, kw)
    beta, Ainv = GR.gls(c["X"], c["y"], ids, G, 0.3)
    # the start is the rho = 0 solve (OLS); the next solve is the GLS one, and it is a fixed point
    two = eng.fit_glm_gee("gaussian", "identity", rho=0.3, max_iter=2)
    three = eng.fit_glm_gee("gaussian", "identity", rho=0.3, max_iter=3)
    cond = float(np.linalg.cond(c["X"].T @ c["X"]))
    check_fit("gls", two.fit, dict(coefs=beta, stderr=np.sqrt(np.diag(Ainv))), cond)
    assert rel(three.fit.coefs, two.fit.coefs) <= 1e-12 and two.rho == 0.3


def test_vcov_gee_converged_and_perturbed(eng):
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    r = eng.fit_glm_gee("poisson", "log")
    for label, beta, rho in (("converged", r.fit.coefs, r.rho), ("perturbed", r.fit.coefs + 0.05, r.rho * 0.7)):
        ref = GR.gee_pass(c["X"], c["y"], beta, ids, G, "poisson", "log", rho=rho, **kw)
        cond = downdate_cond(ref)
        Vn = eng.vcov_gee(beta, rho, "poisson", "log", robust=False)
        want = GR.gee_cov(c["X"], c["y"], beta, rho, ids, G, "poisson", "log", robust=False, **kw)
        e0 = scaled_err(Vn, want["V"])
        print(f"\nMARGIN vcov_gee {label} naive: {v_bar(cond) / max(e0, 1e-300):.3g} (cond {cond:.2e})")
        assert e0 <= v_bar(cond) and np.array_equal(Vn, Vn.T)
        for ca in (True, False):
            want = GR.gee_cov(c["X"], c["y"], beta, rho, ids, G, "poisson", "log", robust=True, cadjust=ca, **kw)
            V, M = eng.vcov_gee(beta, rho, "poisson", "log", cadjust=ca, return_meat=True)
            e, em = scaled_err(V, want["V"]), scaled_err(M, want["M"])
            print(f"MARGIN vcov_gee {label} robust cadjust={ca}: {v_bar(cond) / max(e, 1e-300):.3g} (err {e:.2e}, "
                  f"meat {em:.2e})")
            assert e <= v_bar(cond) and em <= 1e-9 and np.array_equal(V, V.T), (label, ca, e, em)
    # the fit's standard errors are those of inv(A) at the last solve
    naive = eng.vcov_gee(r.fit.coefs, r.rho, "poisson", "log", robust=False) / r.phi
    assert rel(np.sqrt(np.diag(naive)), r.fit.stderr) < 1e-3  # (rho moves linearly: the last solve saw the rho before)


def test_a_group_of_zero_prior_weight(eng):
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    pw = kw["pw"].copy()
    pw[ids == 3] = 0.0
    kw0 = dict(kw, pw=pw)
    load(eng, c, ids, G, kw0)
    ref = check_pass("zero-weight group", eng, c, ids, G, kw0, "poisson", "log", c["beta"] * 0.8)
    got = eng.gee_pass(c["beta"] * 0.8, "poisson", "log")
    assert got["n"][3] == 0.0 and not got["s"][3].any() and got["E"][3] == 0.0 and ref["n"][3] == 0.0
    r = eng.fit_glm_gee("poisson", "log")
    assert r.G_eff == G - 1 and r.N == int(np.sum(pw > 0))
    V, M = eng.vcov_gee(r.fit.coefs, r.rho, "poisson", "log", return_meat=True)
    want = GR.gee_cov(c["X"], c["y"], r.fit.coefs, r.rho, ids, G, "poisson", "log", **kw0)
    assert scaled_err(M, want["M"]) <= 1e-9  # the dead group adds zeros to M


def test_combine_depth(eng):
    """One group of 80 001 one-row segments beside groups of 1 600 rows and a one-segment group: the four scalar
    sums and the row sums go through one, two and three combine levels."""
    n, p = 160_001, 5
    i = np.arange(n)
    ids = np.where(i % 2 == 0, 0, 1 + (i // 2) % 50)
    ids[-1] = 51
    G = 52
    c = GR.make_case("poisson", "log", n, p, ids, G, SEED)
    kw = dict(m=None, off=c["off"], pw=c["pw"])
    load(eng, c, ids, G, kw)
    # (the reference solves the 80 001-row block matrix-free: gee_reference._cg; rho fixed, so that the bar on A
    # is not spent on the estimate's own conditioning over 52 groups)
    check_pass("combine depth", eng, c, ids, G, kw, "poisson", "log", c["beta"] * 0.8, rho=0.002)


def test_refusals(eng):
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    n_max = int(np.bincount(ids).max())
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="n_max"):
        eng.fit_glm_gee("poisson", "log", rho=-1.5 / (n_max - 1))
    with pytest.raises(L.IllegalArgumentException, match="n_max"):
        eng.gee_pass(c["beta"], "poisson", "log", rho=-1.5 / (n_max - 1))
    with pytest.raises(L.IllegalArgumentException, match="below 1"):
        eng.vcov_gee(c["beta"], 1.0, "poisson", "log")
    o, g = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0), L.GeeOpts(7, 0, 0.0)
    assert L.load().sglm_gee_pass(eng._h, C.byref(o), C.byref(g), None, None, None, None, None, None,
                                  None) == L.SGLM_EINVAL
    # one-row clusters only: no within-cluster pair
    eng.set_clusters(np.arange(3001), 3001)
    with pytest.raises(L.IllegalArgumentException, match="pairs"):
        eng.fit_glm_gee("poisson", "log")
    with pytest.raises(L.IllegalArgumentException, match="pairs"):
        eng.gee_pass(c["beta"], "poisson", "log")
    # one cluster of 10 weighted rows: 45 pairs > p = 20 columns, but N = 10 <= p
    pw = np.zeros(3001)
    pw[np.flatnonzero(ids == 2)[:10]] = 1.0
    eng.set_data(c["X"], c["y"], offset=kw["off"], prior=pw)
    eng.set_clusters(ids, G)
    eng.reset_stats()
    for call in (lambda: eng.fit_glm_gee("poisson", "log"), lambda: eng.gee_pass(c["beta"], "poisson", "log"),
                 lambda: eng.vcov_gee(c["beta"], 0.2, "poisson", "log")):
        with pytest.raises(L.IllegalArgumentException, match=r"N = 10, than the p = 20"):
            call()
    assert eng.stats()["passes"] == 0
    load(eng, c, ids, G, kw)  # the handle still works
    check_pass("after the N <= p refusals", eng, c, ids, G, kw, "poisson", "log", c["beta"] * 0.8)
    eng.reset_stats()
    eng.set_clusters(None)
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.fit_glm_gee("poisson", "log")
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.vcov_gee(c["beta"], 0.2, "poisson", "log")
    assert eng.stats()["passes"] == 0  # every refusal came before the first pass
    Xw, yw, _, _ = synth.generate(0, 0, 1000, 257, 3)
    eng.set_data(Xw, yw)
    eng.set_clusters(np.arange(1000) % 7, 7)
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.fit_glm_gee("binomial", "logit")
    eng.synth(0, 0, 4096, 64, 5, procedural=True)
    eng.set_clusters(np.arange(4096) % 7, 7)
    with pytest.raises(L.IllegalArgumentException, match="procedural"):
        eng.fit_glm_gee("binomial", "logit")


def test_a_covariance_that_is_not_finite_is_refused(eng):
    """poisson / identity at a beta whose means are negative: V(mu) < 0, so sqrt(w) is not a number and neither is
    M or V.  SGLM_EINVAL, robust and model-based, exchangeable and independence; the handle works afterwards."""
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    bad = np.zeros(20)
    bad[0] = -1.0  # eta = -1 + offset < 0 on every row
    for corstr, rho in (("exchangeable", 0.2), ("independence", 0.0)):
        for robust in (True, False):
            with pytest.raises(L.IllegalArgumentException, match="not finite.*leaves the family's range"):
                eng.vcov_gee(bad, rho, "poisson", "identity", corstr=corstr, robust=robust)
    good = np.zeros(20)
    good[0] = 3.0
    V = eng.vcov_gee(good, 0.2, "poisson", "identity")
    want = GR.gee_cov(c["X"], c["y"], good, 0.2, ids, G, "poisson", "identity", **kw)
    ref = GR.gee_pass(c["X"], c["y"], good, ids, G, "poisson", "identity", rho=0.2, **kw)
    assert np.all(np.isfinite(V)) and scaled_err(V, want["V"]) <= v_bar(downdate_cond(ref))
    check_pass("after the refusals", eng, c, ids, G, kw, "poisson", "log", c["beta"] * 0.8)


N_BIG, P_BIG = 4001, 64


@pytest.fixture(scope="module")
def big(eng):
    out = {}
    for pat in ("interleaved", "sorted"):
        c, ids, G, kw = case("poisson", "log", N_BIG, P_BIG, pat)
        load(eng, c, ids, G, kw)
        r, o, cond, tol = check_gee_fit(f"big {pat}", eng, c, ids, G, kw, "poisson", "log")
        out[pat] = (c, ids, G, kw, r, cond, tol)
    return out


def test_two_fits_are_bitwise_identical_and_nothing_else_moves(eng, big):
    c, ids, G, kw, one, cond, tol = big["interleaved"]
    load(eng, c, ids, G, kw)
    for r in (eng.fit_glm_gee("poisson", "log", tol=tol), eng.fit_glm_gee("poisson", "log", tol=tol)):
        assert np.array_equal(r.fit.coefs, one.fit.coefs) and r.rho == one.rho and r.phi == one.phi
        assert np.array_equal(r.fit.dev_trace, one.fit.dev_trace) and np.array_equal(r.fit.stderr, one.fit.stderr)
    ms = eng.gee_ms()
    assert len(ms) == 4 and all(v > 0.0 for v in ms)
    # the other entry points around a GEE fit, on the design without its intercept (which the fixed effects absorb)
    eng.set_data(np.asfortranarray(c["X"][:, 1:]), c["y"], offset=kw["off"], prior=kw["pw"])
    pick = lambda d: (d[0], d[1], d[3], d[4])  # X, y, offset, prior (no m was loaded)
    before = pick(eng.get_data())
    plain0 = eng.fit_glm("poisson", "log")
    eng.set_clusters(ids, G)
    fe0 = eng.fit_glm_fe("poisson", "log")
    V0 = eng.vcov_cluster(plain0.coefs, "poisson", "log")
    ids2 = (np.arange(N_BIG) // 3) % 5  # a declared second factor stays declared, and its fit what it was
    eng.set_fe2(ids2, 5)
    two0 = eng.fit_glm_fe2("poisson", "log")
    a = eng.fit_glm_gee("poisson", "log")
    b = eng.fit_glm_gee("poisson", "log")
    assert np.array_equal(a.fit.coefs, b.fit.coefs) and a.rho == b.rho and a.phi == b.phi
    eng.vcov_gee(a.fit.coefs, a.rho, "poisson", "log")
    for x, y in zip(before, pick(eng.get_data())):
        assert np.array_equal(x, y)
    plain1 = eng.fit_glm("poisson", "log")
    assert np.array_equal(plain1.coefs, plain0.coefs) and np.array_equal(plain1.stderr, plain0.stderr)
    assert np.array_equal(plain1.dev_trace, plain0.dev_trace) and plain1.iter == plain0.iter
    two1 = eng.fit_glm_fe2("poisson", "log")
    assert np.array_equal(two1.fit.coefs, two0.fit.coefs) and np.array_equal(two1.alpha, two0.alpha)
    assert np.array_equal(two1.gamma, two0.gamma) and two1.sweeps == two0.sweeps
    fe1 = eng.fit_glm_fe("poisson", "log")
    assert np.array_equal(fe1.fit.coefs, fe0.fit.coefs) and np.array_equal(fe1.alpha, fe0.alpha)
    assert np.array_equal(eng.vcov_cluster(plain0.coefs, "poisson", "log"), V0)


def assert_same_fit(label, r, one, cond):
    want = dict(coefs=one.fit.coefs, stderr=one.fit.stderr, deviance=one.fit.deviance,
                null_deviance=one.fit.null_deviance, pearson=one.fit.pearson, loglik=one.fit.loglik, iter=one.fit.iter)
    check_fit(label, r.fit, want, cond)
    assert rel(r.rho, one.rho) <= 1e-9 and rel(r.phi, one.phi) <= 1e-9 and r.G_eff == one.G_eff


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
@pytest.mark.parametrize("devices", ([0, 0], [0]))
def test_group_handle_matches_the_single_handle(big, devices, pat):
    c, ids, G, kw, one, cond, tol = big[pat]
    with Engine(devices=devices) as g:
        assert g.gee_ms() == (-1.0, -1.0, -1.0, -1.0)
        load(g, c, ids, G, kw)
        a = g.fit_glm_gee("poisson", "log", tol=tol)
        b = g.fit_glm_gee("poisson", "log", tol=tol)
        assert_same_fit(f"group {devices} {pat}", a, one, cond)
        assert np.array_equal(a.fit.coefs, b.fit.coefs) and a.rho == b.rho and a.phi == b.phi


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
def test_local_communicator_ranks_agree(eng, big, pat):
    c, ids, G, kw, one, cond, tol = big[pat]
    load(eng, c, ids, G, kw)
    V1 = eng.vcov_gee(one.fit.coefs, one.rho, "poisson", "log")
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(N_BIG, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(c["X"][lo:hi]), c["y"][lo:hi], offset=kw["off"][lo:hi],
                           prior=kw["pw"][lo:hi])
                e.set_clusters(ids[lo:hi], G)  # global codes
                fit = e.fit_glm_gee("poisson", "log", tol=tol)
                res[r] = (fit, e.vcov_gee(fit.fit.coefs, fit.rho, "poisson", "log"))
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    f0, f1 = res[0][0], res[1][0]
    assert np.array_equal(f0.fit.coefs, f1.fit.coefs) and f0.rho == f1.rho and f0.phi == f1.phi
    assert np.array_equal(f0.fit.dev_trace, f1.fit.dev_trace) and np.array_equal(res[0][1], res[1][1])
    assert_same_fit(f"local comm {pat}", f0, one, cond)
    assert scaled_err(res[0][1], V1) <= v_bar(cond)


def test_python_round_trip_on_iris(iris):
    """GLM.fit_gee with Species as the cluster factor against the reference fit; summary, vcov_gee,
    coeftest(gee=) and predict on the model."""
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    sp = iris["Species"]
    ids = np.unique(sp, return_inverse=True)[1]
    y = Frame({"Sepal_Width": iris["Sepal_Width"]})
    x = Frame({"(Intercept)": np.ones(len(sp)), "Petal_Length": iris["Petal_Length"], "Petal_Width": iris["Petal_Width"]})
    cl = Frame({"Species": sp})
    X = np.asfortranarray(np.column_stack([np.ones(len(sp)), iris["Petal_Length"], iris["Petal_Width"]]))
    yv = np.asarray(iris["Sepal_Width"], dtype=np.float64)
    for fam, lnk in (("gaussian", "identity"), ("gamma", "log")):
        tol = clear_tol(f"iris {fam}/{lnk}", GR.gee_fit(X, yv, ids, 3, fam, lnk, tol=1e-11, max_iter=30)["dev_trace"])
        o = GR.gee_fit(X, yv, ids, 3, fam, lnk, tol=tol)
        obj = GLM.fit_gee(y, x, cl, fam, lnk, tol=tol)
        beta = np.asarray(obj.coefs).reshape(-1)
        assert obj.iter == o["iter"] and obj.corstr == "exchangeable" and obj.aic is None
        assert rel(beta, o["coefs"]) < 1e-8 and rel([obj.rho, obj.scale], [o["rho"], o["phi"]]) < 1e-8
        want = GR.gee_cov(X, yv, beta, obj.rho, ids, 3, fam, lnk)
        assert rel(obj.stdErr, np.sqrt(np.diag(want["V"]))) < 1e-8
        assert rel(obj.naive_se, np.sqrt(o["phi"]) * o["stderr"]) < 1e-8
        text = GLM.summary_string(obj)
        assert "Correlation (exchangeable): " in text and "Scale: " in text and "AIC" not in text
        V = GLM.vcov_gee(obj, y, x, cl)
        assert rel(np.sqrt(np.diag(V)), obj.stdErr) < 1e-12
        Vn = GLM.vcov_gee(obj, y, x, cl, robust=False)
        assert rel(np.sqrt(np.diag(Vn)), np.sqrt(np.diag(GR.gee_cov(X, yv, beta, obj.rho, ids, 3, fam, lnk,
                                                                      robust=False)["V"]))) < 1e-8
        tab = GLM.coeftest(obj, y, x, gee=cl)  # coeftest's cadjust defaults to True: G / (G - 1) = 3 / 2
        assert list(tab["name"]) == obj.xnames
        assert rel(tab["se"], np.sqrt(1.5) * np.asarray(obj.stdErr)) < 1e-12
        same = GLM.coeftest(obj, y, x, gee=cl, cadjust=False)  # the model's own standard errors
        assert rel(same["se"], np.asarray(obj.stdErr)) < 1e-12
        assert rel(tab["stat"], beta / np.asarray(tab["se"])) < 1e-12
        new = Frame({"(Intercept)": np.ones(3), "Petal_Length": np.array([1.5, 4.0, 5.5]),
                     "Petal_Width": np.array([0.2, 1.3, 2.0])})
        eta = np.column_stack([np.ones(3), new["Petal_Length"], new["Petal_Width"]]) @ beta
        assert rel(obj.predict(new)["value"], eta if lnk == "identity" else np.exp(eta)) < 1e-12
