"""The sandwich (HC0-HC3) covariance on the GPU (sglm_vcov_robust: the score-weight kernel of influence.hip
and a Gram pass weighted by its output) against tests/sandwich_reference.py, a numpy reference built by
a different algorithm (QR for h and C, BLAS for M).

Error metric: e = max_ij |V - V_ref|_ij / sqrt(V_ref,ii V_ref,jj).

Bars
  V     e <= max(1e-9, K_BOUND cond eps) (2 + k max_i h_i / (1 - h_i)): the bread's own bar (the leverage
        tests' h_bar), twice because C enters twice, plus the first-order amplification of the leverage's
        bar through (1 - h)^-k.  h is the REFERENCE's, and every test asserts max h_ref <= 0.5, so an easy
        bar can never come from the engine.
  meat  the same metric on M against 1e-9 (1 + k max h / (1 - h)).

Checked on the CPU for exactly the sweep's shapes and seeds (beta after 3 IRLS iterations from
eta0 = logit(mean y)): max h <= 0.376, cond <= 3.4e3, and V by two numpy routes (explicit inverse against
the QR factor) agrees to <= 4.1e-15 -- the 1e-9 bar has >= 1e5 of margin from the reference alone.
"""
import threading

import numpy as np
import pytest

import links_reference as LR
from conftest import K_BOUND, gram_cond, iris_design
from sandwich_reference import HC_POWER, h_amp, sandwich, scaled_err
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
H_MAX = 0.5


def c_bar(cond):
    return max(1e-9, K_BOUND * cond * EPS)


def check(label, eng, X, y, beta, fam, lnk, cond, types=("HC0", "HC3"), **kw):
    out = {}
    for t in types:
        ref = sandwich(X, y, beta, fam, lnk, t, **kw)
        assert float(np.max(ref["h"])) <= H_MAX, (label, float(np.max(ref["h"])))
        amp = h_amp(ref["h"], t)
        V, M = eng.vcov_robust(beta, fam, lnk, type=t, return_meat=True)
        assert np.array_equal(V, V.T), (label, t)
        e_v, e_m = scaled_err(V, ref["V"]), scaled_err(M, ref["M"])
        bar_v, bar_m = c_bar(cond) * (2.0 + amp), 1e-9 * (1.0 + amp)
        print(f"\nMARGIN {label} {t}: {min(bar_v / max(e_v, 1e-300), bar_m / max(e_m, 1e-300)):.3g} "
              f"(V: bar {bar_v:.2e} err {e_v:.2e}; meat: bar {bar_m:.2e} err {e_m:.2e}; cond {cond:.2e}, "
              f"max h {float(np.max(ref['h'])):.3f})")
        assert e_v <= bar_v, (label, t, e_v, bar_v)
        assert e_m <= bar_m, (label, t, e_m, bar_m)
        out[t] = (V, M, ref)
    return out


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


SWEEP_P = (1, 5, 16, 17, 20, 32, 33, 64, 65, 80, 128, 129, 256)


@pytest.mark.parametrize("p", SWEEP_P)
def test_shape_sweep_logit(eng, p):
    """Every pass path (narrow P16 1-4, K1 5-8, K1r 9 and 16) and every score-kernel width, odd block
    counts, row tails that are no multiple of 16 / 32 / 64 / 128, one and many workgroups."""
    types = ("HC0", "HC3", "HC1", "HC2") if p in (20, 129) else ("HC0", "HC3")
    for n in (8 * p + 1, 1000 + 15 * (p % 7)):
        X, y, _, _ = synth.generate(0, 0, n, p, 7 + p)
        eng.set_data(X, y)
        f = eng.fit_glm("binomial", "logit", max_iter=3)
        cond = gram_cond(eng, f.coefs)
        check(f"sweep {n}x{p}", eng, X, y, f.coefs, "binomial", "logit", cond, types)


def family_case(name, n=3001, p=20):
    rng = np.random.default_rng(5)
    if name.startswith("binomial"):
        X, _, _, _ = synth.generate(0, 0, n, p, 11)
        m = rng.integers(5, 10, n).astype(np.float64)  # mean(y) < min(m): the fit starts at mu = mean(y) for every row
        pr = np.clip(0.5 + 0.25 * (X @ synth.beta_star(p)), 0.05, 0.95)
        y = rng.binomial(m.astype(int), pr).astype(np.float64)
        return X, y, dict(m=m), "binomial", name.split("/")[1]
    if name == "poisson/sqrt":  # the non-canonical pair, on the link tests' own design (valid mu = eta^2)
        X, y, off, prior = LR.make_case("poisson", n, p)
        return X, y, dict(off=off, pw=prior), "poisson", "sqrt"
    if name == "poisson":
        X, y, off, prior = synth.generate(2, 0, n, p, 11)
        return X, y, dict(off=off, pw=prior), "poisson", "log"
    if name == "gamma":
        X, y, _, _ = synth.generate(3, 0, n, p, 11)
        return X, y, {}, "gamma", "inverse"
    X, y, _, _ = synth.generate(1, 0, n, p, 11)
    return X, y, {}, "gaussian", "identity"


@pytest.mark.parametrize("name", ["binomial/logit", "binomial/probit", "binomial/cloglog", "poisson", "gamma",
                                  "gaussian", "poisson/sqrt"])
def test_every_family_link(eng, name):
    X, y, kw, fam, lnk = family_case(name)
    eng.set_data(X, y, m=kw.get("m"), offset=kw.get("off"), prior=kw.get("pw"))
    f = eng.fit_glm(fam, lnk)
    cond = gram_cond(eng, f.coefs, fam, lnk)
    check(name, eng, X, y, f.coefs, fam, lnk, cond, **kw)


def test_algebra(eng):
    n, p = 3001, 20
    X, y, _, _ = synth.generate(0, 0, n, p, 4)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit")
    v0, m0 = eng.vcov_robust(f.coefs, "binomial", "logit", type="HC0", return_meat=True)
    v1 = eng.vcov_robust(f.coefs, "binomial", "logit", type="HC1")
    assert np.all(np.abs(v1 - v0 * (n / (n - p))) <= 1e-14 * np.abs(v1))
    mu = 1.0 / (1.0 + np.exp(-(X @ f.coefs)))
    u = y - mu  # logit: w g' = 1
    want = X.T @ ((u * u)[:, None] * X)
    assert scaled_err(m0, want) <= 1e-9
    for t in L.HC_TYPES:
        V = eng.vcov_robust(f.coefs, "binomial", "logit", type=t)
        assert np.array_equal(V, V.T), t
    assert np.array_equal(eng.vcov_robust(f.coefs, "binomial", "logit", type="HC0"), v0)  # return_meat changes nothing
    s, m = eng.sandwich_ms()
    assert s > 0.0 and m > 0.0


def test_glm_vcov_const_is_bitwise_the_engines_vcov(eng):
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    X, y, _, _ = synth.generate(0, 0, 3001, 5, 2)
    names = [f"x{j}" for j in range(5)]
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    obj = GLM.fit(yf, xf, "binomial", "logit")
    beta = np.asarray(obj.coefs).reshape(-1)
    eng.set_data(X, y)
    C = eng.vcov(beta, "binomial", "logit")
    assert np.array_equal(GLM.vcov(obj, yf, xf), C)
    assert np.array_equal(GLM.vcov(obj, yf, xf, type="const"), C)
    ref = sandwich(X, y, beta, "binomial", "logit", "HC3")
    cond = float(np.linalg.cond(np.linalg.inv(C)))
    assert scaled_err(GLM.vcov(obj, yf, xf, type="HC3"), ref["V"]) <= c_bar(cond) * (2.0 + h_amp(ref["h"], "HC3"))
    t = GLM.coeftest(obj, yf, xf)
    se = np.sqrt(np.diag(ref["V"]))
    assert t.columns == ["name", "estimate", "se", "stat", "pvalue"] and list(t["name"]) == names
    assert np.all(np.abs(t["se"] - se) <= 1e-9 * se)
    assert np.array_equal(t["stat"], beta / t["se"])


def test_lm_on_iris(iris):
    from scipy import stats
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.lm import LM
    X, y, names = iris_design(iris)
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    obj = LM.fit(xf, yf)
    beta = np.asarray(obj.coefs).reshape(-1)
    cond = float(np.linalg.cond(X.T @ X))
    for t in ("HC0", "HC3"):
        ref = sandwich(X, y, beta, "gaussian", "identity", t)
        assert float(np.max(ref["h"])) <= H_MAX
        e = y - X @ beta  # White / HC3 written out
        XtXi = np.linalg.inv(X.T @ X)
        white = XtXi @ (X.T @ ((e * e / (1.0 - ref["h"]) ** HC_POWER[t])[:, None] * X)) @ XtXi
        assert scaled_err(white, ref["V"]) <= 1e-12
        V = LM.vcov(obj, xf, yf, type=t)
        err, bar = scaled_err(V, ref["V"]), c_bar(cond) * (2.0 + h_amp(ref["h"], t))
        print(f"\nMARGIN LM iris {t}: {bar / max(err, 1e-300):.3g}")
        assert err <= bar
    const = LM.vcov(obj, xf, yf)
    want = obj.sigma ** 2 * np.linalg.inv(X.T @ X)
    assert scaled_err(const, want) <= c_bar(cond)
    tab = LM.coeftest(obj, xf, yf)  # HC3
    se = np.sqrt(np.diag(ref["V"]))
    assert list(tab["name"]) == names and np.array_equal(tab["estimate"], beta)
    assert np.all(np.abs(tab["se"] - se) <= bar * se)
    assert np.array_equal(tab["stat"], beta / tab["se"])
    assert np.allclose(tab["pvalue"], 2.0 * stats.t.sf(np.abs(tab["stat"]), len(y) - 4), rtol=0, atol=1e-12)


def test_zero_prior_weights(eng):
    X, y, off, prior = synth.generate(2, 0, 3001, 20, 6)
    prior = prior.copy()
    dead = np.arange(3001) % 7 == 3
    prior[dead] = 0.0
    keep = ~dead
    eng.set_data(X, y, offset=off, prior=prior)
    f = eng.fit_glm("poisson", "log")
    cond = gram_cond(eng, f.coefs, "poisson", "log")
    full = check("zero prior", eng, X, y, f.coefs, "poisson", "log", cond, ("HC0", "HC2", "HC3"), off=off, pw=prior)
    eng.set_data(np.asfortranarray(X[keep]), y[keep], offset=off[keep], prior=prior[keep])
    for t in ("HC0", "HC2", "HC3"):  # (HC1's n differs by definition)
        part = eng.vcov_robust(f.coefs, "poisson", "log", type=t)
        V, _, ref = full[t]
        assert np.all(ref["omega"][dead] == 0.0)
        err, bar = scaled_err(V, part), c_bar(cond) * (2.0 + h_amp(ref["h"][keep], t))
        assert err <= bar, (t, err, bar)


N_BIG, P_BIG = 70_001, 64


@pytest.fixture(scope="module")
def big(eng):
    X, y, _, _ = synth.generate(0, 0, N_BIG, P_BIG, 21)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit")
    cond = gram_cond(eng, f.coefs)
    one = {t: eng.vcov_robust(f.coefs, "binomial", "logit", type=t, return_meat=True) for t in ("HC1", "HC3")}
    return X, y, f, cond, one


def test_two_calls_are_bitwise_identical_and_the_shard_is_untouched(eng, big):
    X, y, f, cond, one = big
    eng.set_data(X, y)
    before = eng.get_data()[:2]
    fit0 = eng.fit_glm("binomial", "logit")
    for t in ("HC1", "HC3"):
        V, M = eng.vcov_robust(f.coefs, "binomial", "logit", type=t, return_meat=True)
        assert np.array_equal(V, one[t][0]) and np.array_equal(M, one[t][1]), t
    after = eng.get_data()[:2]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(before[0], X) and np.array_equal(before[1], y)
    fit1 = eng.fit_glm("binomial", "logit")
    assert np.array_equal(fit0.coefs, fit1.coefs) and np.array_equal(fit0.stderr, fit1.stderr)
    assert fit0.deviance == fit1.deviance and fit0.iter == fit1.iter
    assert np.array_equal(fit0.coefs, f.coefs)
    # the fit's kernel record is the fit's, not the meat pass's
    name = eng.stats()["pass_kernel_name"]
    eng.vcov_robust(f.coefs, "binomial", "logit", type="HC0")
    assert eng.stats()["pass_kernel_name"] == name


def test_big_against_the_reference(eng, big):
    X, y, f, cond, one = big
    for t in ("HC1", "HC3"):
        ref = sandwich(X, y, f.coefs, "binomial", "logit", t)
        assert float(np.max(ref["h"])) <= H_MAX
        err, bar = scaled_err(one[t][0], ref["V"]), c_bar(cond) * (2.0 + h_amp(ref["h"], t))
        print(f"\nMARGIN big {t}: {bar / max(err, 1e-300):.3g}")
        assert err <= bar


def test_group_handle_matches_the_single_handle(big):
    X, y, f, cond, one = big
    with Engine(devices=[0, 0]) as g:
        g.set_data(X, y)
        for t in ("HC1", "HC3"):  # HC1: n is the global 70 001
            V = g.vcov_robust(f.coefs, "binomial", "logit", type=t)
            assert scaled_err(V, one[t][0]) <= c_bar(cond), t
            assert np.array_equal(V, V.T)
        s, m = g.sandwich_ms()
        assert s > 0.0 and m > 0.0


def test_local_communicator_ranks_agree(big):
    X, y, f, cond, one = big
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(N_BIG, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi])
                res[r] = {t: e.vcov_robust(f.coefs, "binomial", "logit", type=t) for t in ("HC1", "HC3")}
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    for t in ("HC1", "HC3"):
        assert np.array_equal(res[0][t], res[1][t]), t
        assert scaled_err(res[0][t], one[t][0]) <= c_bar(cond), t


def test_refusals(eng):
    X, y, _, _ = synth.generate(0, 0, 1000, 272, 3)
    eng.set_data(X, y)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.vcov_robust(np.zeros(272), "binomial", "logit")
    assert eng.stats()["passes"] == 0  # refused before any launch
    eng.synth(0, 0, 4096, 64, 5, procedural=True)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="procedural"):
        eng.vcov_robust(np.zeros(64), "binomial", "logit")
    assert eng.stats()["passes"] == 0
    X, y, _, _ = synth.generate(1, 0, 5000, 6, 3)
    eng.set_data(np.column_stack([X, X[:, 2]]), y)
    with pytest.raises(L.MatrixSingularException):
        eng.vcov_robust(np.zeros(7), "gaussian", "identity")
