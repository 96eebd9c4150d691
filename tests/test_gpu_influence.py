"""Per-row diagnostics on the GPU (sglm_vcov / sglm_influence / sglm_predict_new_se; influence.hip)
against numpy references built by a different algorithm:

  h_ref   = rowsum(Q^2), Q from np.linalg.qr(sqrt(w) X)          (the engine inverts X'WX explicitly)
  w, mu, residuals from the formulas of include/sglm.h in numpy (oracle/np_reference's row functions)

Bars
  h          per row |h - h_ref| / h_ref <= max(1e-9, K_BOUND cond eps); rows with prior weight 0 give
             exactly 0.  QR and an explicit inverse agree to 4e-15 (logit, LM, poisson) / 9e-13 (gamma)
             on these designs, so the fixed 1e-9 has >= 1e3 of margin from the reference alone.
  residuals  |d| <= 1e-9 (|r_ref| + s_i), s_i the residual's formula with (y - mu) replaced by
             |y| + |mu| (the scale before the cancellation in y - mu).  Deviance residuals are compared
             as signed squares against sign(y - mu) factor unit_dev with the floor 1e-9 (|y| + |mu|):
             the sqrt near y = mu amplifies the unit deviance's cancellation by ~1 / sqrt(eps), between
             two CPU implementations of the formula already.  Signs must match where
             |y - mu| > 1e-9 (|y| + |mu|).

The n = 2p and 2p + 1 shapes of the sweep are linearly separable (n points in p dimensions), so the
logit MLE does not exist there: an uncapped IRLS runs the coefficients off until the weights
underflow (numpy, p = 16, n = 32 after 8 iterations: |eta| = 52, min w = 3e-23, and QR against the
explicit inverse -- two CPU implementations -- already part by 1e-8; p = 17 ends in NaN).  Those
shapes therefore take the coefficients after 3 IRLS iterations (|eta| <= 19, min w >= 5e-9, cond <=
3e4; numpy's QR and explicit inverse agree to 7e-13 there); every other shape is fitted to
convergence.  The shapes and every bar are unchanged.
"""
import threading

import numpy as np
import pytest

import np_reference as R
from conftest import K_BOUND, gram_cond, iris_design
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
RESIDS = ("response", "working", "pearson", "deviance")


def reference(X, y, beta, fam, lnk, m=None, off=None, pw=None):
    """w, h (QR), the four residuals with their scales, mu -- numpy, independent of the engine."""
    n = len(y)
    m = np.ones(n) if m is None else m
    off = np.zeros(n) if off is None else off
    pw = np.ones(n) if pw is None else pw
    eta = X @ beta + off
    mu = R.unlink(fam, lnk, eta, m)
    g = R.lprime(fam, lnk, mu, m)
    v = R.variance(fam, mu, m)
    w = pw / (v * g * g)
    Q, _ = np.linalg.qr(np.sqrt(w)[:, None] * X)
    h = np.sum(Q * Q, axis=1)
    e, s = y - mu, np.abs(y) + np.abs(mu)
    sp = np.sqrt(pw / v)
    res = {"response": (e, s), "working": (e * g, s * np.abs(g)), "pearson": (e * sp, s * sp),
           "deviance": (np.sign(e) * R.dev_factor(fam) * R.dev_rows(fam, y, mu, m, pw), s)}
    return dict(w=w, h=h, res=res, mu=mu, e=e, s=s, pw=pw)


def h_bar(cond):
    return max(1e-9, K_BOUND * cond * EPS)


def check_hat(label, h, ref, cond):
    zero = ref["pw"] == 0.0
    assert np.all(h[zero] == 0.0), label
    err = np.abs(h[~zero] - ref["h"][~zero]) / ref["h"][~zero]
    bar = h_bar(cond)
    worst = float(err.max()) if err.size else 0.0
    print(f"\nMARGIN {label}: {bar / max(worst, 1e-300):.3g} (hat: bar {bar:.2e}, cond {cond:.2e}, max err {worst:.2e})")
    assert worst <= bar, (label, worst, bar)


def check_resid(label, kind, r, ref):
    want, scale = ref["res"][kind]
    if kind == "deviance":
        got = np.sign(r) * r * r
        # (a row with prior weight 0 has the deviance residual 0 whatever y - mu is: no sign to match)
        big = (np.abs(ref["e"]) > 1e-9 * ref["s"]) & (ref["pw"] > 0.0)
        assert np.all(np.sign(r[big]) == np.sign(ref["e"][big])), (label, kind)
    else:
        got = r
    err = np.abs(got - want)
    bar = 1e-9 * (np.abs(want) + scale)
    ok = err <= bar
    worst = float(np.max(err / np.maximum(bar, 1e-300))) if err.size else 0.0
    print(f"MARGIN {label} {kind}: {1.0 / max(worst, 1e-300):.3g}")
    assert np.all(ok), (label, kind, worst)


def check_all(label, eng, X, y, beta, fam, lnk, cond, m=None, off=None, pw=None, sum_to=None):
    ref = reference(X, y, beta, fam, lnk, m, off, pw)
    first = None
    for kind in RESIDS:
        inf = eng.influence(beta, fam, lnk, resid=kind)
        check_resid(label, kind, inf.resid, ref)
        if first is None:
            first = inf
            check_hat(label, inf.hat, ref, cond)
            if sum_to is not None:
                assert abs(inf.sum_hat - sum_to) <= 1e-9 * sum_to, (label, inf.sum_hat, sum_to)
        else:  # h and Cook's distance do not depend on the residual type asked for
            assert np.array_equal(inf.hat, first.hat) and np.array_equal(inf.cooks, first.cooks), (label, kind)
    return first, ref


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


SWEEP_P = (1, 5, 16, 17, 20, 32, 33, 64, 65, 80, 128, 129, 256)


def sweep_rows(p):
    ns = [2 * p, 2 * p + 1, 1000 + 15 * (p % 7)]
    if p in (20, 64, 256):
        ns.append(70_001)
    return ns


def sweep_seed(p, n):
    # p = 1 (an intercept alone): the seed is chosen so that y is not constant (mean(y) in {0, 1} has no logit)
    return 12 if p == 1 and n <= 3 else 7 + p


@pytest.mark.parametrize("p", SWEEP_P)
def test_shape_sweep_logit(eng, p):
    """Every P16 boundary, odd block counts, both row-block widths of the kernel, row tails that are no
    multiple of 16 / 64 / 128, one and many workgroups."""
    for n in sweep_rows(p):
        X, y, _, _ = synth.generate(0, 0, n, p, sweep_seed(p, n))
        eng.set_data(X, y)
        f = eng.fit_glm("binomial", "logit", max_iter=3 if n <= 2 * p + 1 else 0)
        cond = gram_cond(eng, f.coefs)
        check_all(f"sweep {n}x{p}", eng, X, y, f.coefs, "binomial", "logit", cond, sum_to=float(p))


def family_case(name, n=3001, p=20):
    rng = np.random.default_rng(5)
    if name.startswith("binomial"):
        X, _, _, _ = synth.generate(0, 0, n, p, 11)
        m = rng.integers(5, 10, n).astype(np.float64)  # mean(y) < min(m): the fit starts at mu = mean(y) for every row
        pr = np.clip(0.5 + 0.25 * (X @ synth.beta_star(p)), 0.05, 0.95)
        y = rng.binomial(m.astype(int), pr).astype(np.float64)
        return X, y, dict(m=m), "binomial", name.split("/")[1]
    if name == "poisson":
        X, y, off, prior = synth.generate(2, 0, n, p, 11)
        return X, y, dict(off=off, pw=prior), "poisson", "log"
    if name == "gamma":
        X, y, _, _ = synth.generate(3, 0, n, p, 11)
        return X, y, {}, "gamma", "inverse"
    X, y, _, _ = synth.generate(1, 0, n, p, 11)
    return X, y, {}, "gaussian", "identity"


@pytest.mark.parametrize("name", ["binomial/logit", "binomial/probit", "binomial/cloglog", "poisson", "gamma",
                                  "gaussian"])
def test_every_family_link(eng, name):
    X, y, kw, fam, lnk = family_case(name)
    eng.set_data(X, y, m=kw.get("m"), offset=kw.get("off"), prior=kw.get("pw"))
    f = eng.fit_glm(fam, lnk)
    cond = gram_cond(eng, f.coefs, fam, lnk)
    check_all(name, eng, X, y, f.coefs, fam, lnk, cond, sum_to=float(X.shape[1]), **kw)


@pytest.mark.parametrize("kind,fam,lnk", [(0, "binomial", "logit"), (2, "poisson", "log"), (3, "gamma", "inverse")])
def test_ties_to_the_fit_summaries(eng, kind, fam, lnk):
    """Sum of squared Pearson / deviance residuals = the fit's Pearson chi^2 / deviance (both pinned
    against the oracle elsewhere) at the fitted coefficients; sqrt(diag(vcov)) = the fit's standard
    errors.  Those are sqrt(diag(inv(X'WX))) of the fit's LAST SOLVE (GLM.scala:307 / 464), whose X'WX
    was formed at the coefficients of the iteration before the returned ones -- so vcov is taken there
    (the same fit stopped one iteration earlier, bitwise the same path).  numpy's restatement of the
    reference shows the same: its stderr equals the inverse at the previous iterate to 3e-16 .. 1e-14
    and parts from the inverse at the returned coefficients by 1.3e-9 (logit) to 5e-6 (poisson, gamma),
    the last step's effect on W; the engine's fit run to a deviance that no longer changes (tol = 0)
    still parts by 2.5e-11 (poisson) there."""
    X, y, off, prior = synth.generate(kind, 0, 20_000, 64, 3)
    eng.set_data(X, y, offset=off, prior=prior)
    f = eng.fit_glm(fam, lnk)
    assert f.iter >= 2
    prev = eng.fit_glm(fam, lnk, max_iter=f.iter - 1)  # the coefficients the last solve's X'WX was formed at
    rp = eng.influence(f.coefs, fam, lnk, resid="pearson").resid
    rd = eng.influence(f.coefs, fam, lnk, resid="deviance").resid
    se = np.sqrt(np.diag(eng.vcov(prev.coefs, fam, lnk)))
    e_p = abs(float(np.sum(rp * rp)) - f.pearson) / f.pearson
    e_d = abs(float(np.sum(rd * rd)) - f.deviance) / f.deviance
    e_s = float(np.max(np.abs(se - f.stderr) / f.stderr))
    print(f"\nMARGIN ties {fam}: pearson {1e-9 / max(e_p, 1e-300):.3g}, deviance {1e-9 / max(e_d, 1e-300):.3g}, "
          f"stderr {1e-12 / max(e_s, 1e-300):.3g} [{e_s:.2e}]")
    assert e_p <= 1e-9 and e_d <= 1e-9
    assert e_s <= 1e-12


@pytest.mark.parametrize("kind,fam,lnk,p", [(0, "binomial", "logit", 20), (0, "binomial", "logit", 129),
                                            (3, "gamma", "inverse", 64)])
def test_vcov_inverts_the_engines_gramian(eng, kind, fam, lnk, p):
    X, y, _, _ = synth.generate(kind, 0, 5000, p, 9)
    eng.set_data(X, y)
    f = eng.fit_glm(fam, lnk)
    G, _, _ = eng.irls_pass(f.coefs, family=fam, link=lnk)
    cond = float(np.linalg.cond(G))
    C = eng.vcov(f.coefs, fam, lnk)
    ref = np.linalg.inv(G)
    err = float(np.max(np.abs(C - ref)) / np.max(np.abs(ref)))
    bar = h_bar(cond)
    print(f"\nMARGIN vcov {fam} p{p}: {bar / max(err, 1e-300):.3g} (cond {cond:.2e})")
    assert err <= bar
    assert np.array_equal(C, C.T) or float(np.max(np.abs(C - C.T)) / np.max(np.abs(C))) <= bar


def test_cooks_distance(eng):
    X, y, off, prior = synth.generate(2, 0, 3001, 20, 4)
    eng.set_data(X, y, offset=off, prior=prior)
    f = eng.fit_glm("poisson", "log")
    a = eng.influence(f.coefs, "poisson", "log", resid="pearson", dispersion=1.0)
    want = (a.resid / (1.0 - a.hat)) ** 2 * a.hat / (1.0 * 20)
    assert np.all(np.abs(a.cooks - want) <= 1e-12 * np.abs(want))
    b = eng.influence(f.coefs, "poisson", "log", resid="deviance", dispersion=1.0)
    assert np.array_equal(a.cooks, b.cooks)
    phi = 2.5  # the dispersion divides, nothing else
    c = eng.influence(f.coefs, "poisson", "log", resid="pearson", dispersion=phi)
    assert np.all(np.abs(c.cooks - want / phi) <= 1e-12 * np.abs(want))


def test_gamma_dispersion_through_glm_influence():
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    X, y, _, _ = synth.generate(3, 0, 3001, 20, 4)
    names = [f"x{j}" for j in range(20)]
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    obj = GLM.fit(yf, xf, "gamma", "inverse")
    assert obj.pDispersion > 0 and abs(obj.pDispersion - 1.0) > 1e-3
    inf = GLM.influence(obj, yf, xf, type="pearson")
    ref = reference(X, y, np.asarray(obj.coefs).reshape(-1), "gamma", "inverse")
    want = (inf.resid / (1.0 - inf.hat)) ** 2 * inf.hat / (obj.pDispersion * 20)
    assert np.all(np.abs(inf.cooks - want) <= 1e-12 * np.abs(want))
    check_resid("GLM.influence gamma", "pearson", inf.resid, ref)
    assert GLM.vcov(obj, yf, xf).shape == (20, 20)


N_BIG, P_BIG = 70_001, 64


@pytest.fixture(scope="module")
def big(eng):
    X, y, _, _ = synth.generate(0, 0, N_BIG, P_BIG, 21)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit")
    return X, y, f.coefs, eng.influence(f.coefs, "binomial", "logit")


def close12(a, b):
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.abs(b)))


def test_two_calls_are_bitwise_identical(eng, big):
    X, y, beta, one = big
    eng.set_data(X, y)
    two = eng.influence(beta, "binomial", "logit")
    for k in ("hat", "resid", "cooks"):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert one.sum_hat == two.sum_hat


def test_group_handle_matches_the_single_handle(big):
    X, y, beta, one = big
    with Engine(devices=[0, 0]) as g:
        g.set_data(X, y)
        two = g.influence(beta, "binomial", "logit")
    for k in ("hat", "resid", "cooks"):
        assert close12(getattr(two, k), getattr(one, k)), k
    assert abs(two.sum_hat - one.sum_hat) <= 1e-12 * one.sum_hat


def test_local_communicator_ranks_return_their_own_rows(big):
    X, y, beta, one = big
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(N_BIG, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi])
                res[r] = (lo, hi, e.influence(beta, "binomial", "logit"))
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    for r in range(2):
        lo, hi, inf = res[r]
        for k in ("hat", "resid", "cooks"):
            assert close12(getattr(inf, k), getattr(one, k)[lo:hi]), (r, k)
    assert abs(res[0][2].sum_hat + res[1][2].sum_hat - one.sum_hat) <= 1e-12 * one.sum_hat


def test_zero_prior_weights(eng):
    X, y, off, prior = synth.generate(2, 0, 3001, 20, 6)
    prior = prior.copy()
    dead = np.arange(3001) % 7 == 3
    prior[dead] = 0.0
    eng.set_data(X, y, offset=off, prior=prior)
    f = eng.fit_glm("poisson", "log")
    cond = gram_cond(eng, f.coefs, "poisson", "log")
    full, _ = check_all("zero prior", eng, X, y, f.coefs, "poisson", "log", cond, off=off, pw=prior, sum_to=20.0)
    assert np.all(full.hat[dead] == 0.0) and np.all(full.cooks[dead] == 0.0)
    keep = ~dead
    eng.set_data(np.asfortranarray(X[keep]), y[keep], offset=off[keep], prior=prior[keep])
    f2 = eng.fit_glm("poisson", "log")
    part = eng.influence(f2.coefs, "poisson", "log")
    err = float(np.max(np.abs(full.hat[keep] - part.hat) / part.hat))
    assert err <= h_bar(cond), err


@pytest.mark.parametrize("p", [20, 256])
def test_predict_new_se(eng, p):
    X, y, _, _ = synth.generate(0, 0, 4 * p + 1000, p, 13)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit")
    cond = gram_cond(eng, f.coefs)
    C = eng.vcov(f.coefs, "binomial", "logit")
    before = eng.get_data()[:2]  # X, y (no m / offset / prior on this shard)
    phi = 1.7
    for n_new in (1, 17, 5000):
        Xn, _, _, _ = synth.generate(0, 10_000, n_new, p, 14)
        se = eng.predict_new_se(Xn, C, phi)
        want = np.sqrt(phi * np.einsum("ij,ij->i", Xn @ C, Xn))
        err = float(np.max(np.abs(se - want) / want))
        print(f"\nMARGIN predict_new_se {n_new}x{p}: {h_bar(cond) / max(err, 1e-300):.3g}")
        assert err <= h_bar(cond), (n_new, err)
    after = eng.get_data()[:2]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_glm_predict_se_column(eng):
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM, _dmu_deta
    X, y, _, _ = synth.generate(0, 0, 3001, 5, 2)
    names = [f"x{j}" for j in range(5)]
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    obj = GLM.fit(yf, xf, "binomial", "logit")
    C = GLM.vcov(obj, yf, xf)
    beta = np.asarray(obj.coefs).reshape(-1)
    link = obj.predict(xf, type="link", cov=C)
    resp = obj.predict(xf, type="response", cov=C)
    want = np.sqrt(np.einsum("ij,ij->i", X @ C, X))
    assert np.all(np.abs(link["se"] - want) <= 1e-9 * want)
    assert np.all(np.abs(resp["se"] - want * _dmu_deta("logit", X @ beta)) <= 1e-9 * resp["se"])
    assert obj.predict(xf).columns == ["index", "value"]


def test_lm_influence_on_iris(iris):
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.lm import LM
    X, y, names = iris_design(iris)
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    obj = LM.fit(xf, yf)
    inf = LM.influence(obj, xf, yf)
    beta = np.asarray(obj.coefs).reshape(-1)
    Q, _ = np.linalg.qr(X)
    h = np.sum(Q * Q, axis=1)
    cond = float(np.linalg.cond(X.T @ X))
    assert float(np.max(np.abs(inf.hat - h) / h)) <= h_bar(cond)
    assert abs(inf.sum_hat - 4.0) <= 1e-9 * 4.0
    e = y - X @ beta
    cooks = (e / (1.0 - h)) ** 2 * h / (obj.sigma ** 2 * 4)
    de = 1e-9 * (np.abs(e) + np.abs(y) + np.abs(X @ beta))  # the residual bar
    assert np.all(np.abs(inf.resid - e) <= de)
    # Cook's distance (e / (1 - h))^2 h / (sigma^2 p) to first order in the bars of its two inputs:
    # h within h_bar (d log D / d log h = 1 + 2 h / (1 - h)), e within de
    k = h / ((1.0 - h) ** 2 * obj.sigma ** 2 * 4)
    bar = cooks * h_bar(cond) * (1.0 + 2.0 * h / (1.0 - h)) + k * (2.0 * np.abs(e) * de + de * de)
    assert np.all(np.abs(inf.cooks - cooks) <= bar)
    pre = LM.fit_components(xf, yf)
    se = obj.predict(xf, xtxi=pre.xtxi)["se"]
    assert np.all(np.abs(se - obj.sigma * np.sqrt(h)) <= h_bar(cond) * se)


def test_refusals(eng):
    X, y, _, _ = synth.generate(0, 0, 1000, 272, 3)
    eng.set_data(X, y)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.influence(np.zeros(272), "binomial", "logit")
    assert eng.stats()["passes"] == 0  # refused before any launch
    eng.synth(0, 0, 4096, 64, 5, procedural=True)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="procedural"):
        eng.influence(np.zeros(64), "binomial", "logit")
    assert eng.stats()["passes"] == 0
    X, y, _, _ = synth.generate(1, 0, 5000, 6, 3)
    eng.set_data(np.column_stack([X, X[:, 2]]), y)
    with pytest.raises(L.MatrixSingularException):
        eng.influence(np.zeros(7), "gaussian", "identity")
    with pytest.raises(L.MatrixSingularException):
        eng.vcov(np.zeros(7), "gaussian", "identity")
