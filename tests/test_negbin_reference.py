"""tests/negbin_reference.py pinned to the likelihood itself (no GPU).

The reference project has no negative binomial, so the numpy restatement the GPU tests compare against is
itself checked here against properties that do not depend on how it is written: the beta score vanishes at
its fixed-theta fits, its theta score and information are the derivatives of its own log-likelihood (built on
scipy's gammaln), the theta score vanishes at glm_nb's result, and theta -> infinity gives the Poisson fit."""
import numpy as np
import pytest
from scipy.special import gammaln

import links_reference as LR
import negbin_reference as NB

EPS = np.finfo(float).eps


@pytest.mark.parametrize("lnk,theta", [("log", 0.5), ("log", 50.0), ("sqrt", 3.0), ("identity", 3.0)])
def test_beta_score_vanishes_at_the_fixed_theta_fit(lnk, theta):
    """X' [pw (y - mu) / (V g')] = 0 at the maximum of the likelihood in beta: norm-wise against sum |terms|."""
    X, y, off, pw, _ = NB.make_case(lnk, 2001, 7, 2.0, 3)
    f = NB.fit_glm(X, y, theta, lnk, offset=off, prior=pw, tol=1e-12, max_iter=60)
    assert max(f.invalid) == 0
    g = LR.lprime("negbin", lnk, f.mu, 1.0)
    terms = X * (pw * (y - f.mu) / (NB.variance(f.mu, theta) * g))[:, None]
    ratio = np.abs(terms.sum(axis=0)) / np.abs(terms).sum(axis=0)
    print(f"\nbeta score {lnk} theta {theta}: max |sum| / sum|terms| = {ratio.max():.2e} after {f.iter} iterations")
    # Fisher scoring stops at |delta deviance| <= 1e-12: the remaining step is below 1e-6 relative, and the
    # score is linear in the step
    assert ratio.max() < 1e-7


@pytest.mark.parametrize("theta", [0.3, 2.0, 40.0])
def test_theta_score_and_info_are_the_derivatives_of_the_loglik(theta):
    X, y, off, pw, beta = NB.make_case("log", 1501, 5, 2.0, 4)
    mu = np.exp(X @ beta + off)
    pw = pw.copy()
    pw[::7] = 0.0
    ll = lambda t: NB.loglik(y, mu, pw, t)
    score, info, l0, _, sw, _ = NB.theta_terms(y, mu, pw, theta)
    # (theta_terms sums the rows of positive weight only: the same terms in another order, n eps apart at most)
    assert abs(l0 - ll(theta)) <= len(y) * EPS * abs(l0) and abs(sw - pw.sum()) <= len(y) * EPS * sw
    h = theta * 1e-4
    d1 = (ll(theta + h) - ll(theta - h)) / (2 * h)
    d2 = (ll(theta + h) - 2 * ll(theta) + ll(theta - h)) / (h * h)
    e1 = abs(score - d1) / max(abs(d1), 1e-300)
    e2 = abs(-info - d2) / max(abs(d2), 1e-300)
    # The bars: the differences' truncation, O((h / theta)^2) = 1e-8 relative (1e-6 allowed), plus the rounding of
    # the log-likelihood they difference -- each evaluation is a sum of terms that cancel (lgamma(theta + y)
    # against lgamma(theta) and (theta + y) log(theta + mu)), so it carries up to eps * T with T the sum of the
    # terms' absolute values; a first difference divides 2 of them by 2h, a second difference 4 by h^2.
    T = float(np.sum(pw * (np.abs(gammaln(theta + y)) + abs(gammaln(theta)) + gammaln(y + 1.0)
                           + abs(theta * np.log(theta)) + np.abs(y * np.log(mu))
                           + (theta + y) * np.abs(np.log(theta + mu)))))
    bar1 = 1e-6 + EPS * T / h / abs(d1)
    bar2 = 1e-6 + 4 * EPS * T / (h * h) / abs(d2)
    print(f"\ntheta {theta}: score {score:.6g} vs {d1:.6g} ({e1:.1e}, bar {bar1:.1e}); info {info:.6g} vs {-d2:.6g} "
          f"({e2:.1e}, bar {bar2:.1e})")
    assert e1 < bar1
    assert e2 < bar2


@pytest.mark.parametrize("lnk,theta_star", [("log", 2.0), ("sqrt", 3.0)])
def test_theta_score_vanishes_at_glm_nb(lnk, theta_star):
    X, y, off, pw, _ = NB.make_case(lnk, 4001, 6, theta_star, 5)
    r = NB.glm_nb(X, y, lnk, offset=off, prior=pw, tol=1e-9)
    assert r.converged and all(t.warn == 0 for t in r.theta_runs)
    score, info, ll, _, _, norm = NB.theta_terms(y, r.fit.mu, pw, r.theta)
    last = abs(r.theta_runs[-1].dels[-1])
    # Newton: after a step del the score is ~ info del^2 l''' / (2 l'') -- bounded here by info * |del| itself
    print(f"\nglm_nb {lnk}: theta {r.theta:.6f} (true {theta_star}), se {r.se_theta:.4f}, outer {r.outer_iter}, "
          f"score {score:.2e}, info |del| {info * last:.2e}, norm {norm:.3g}")
    assert abs(score) <= info * last + 1e-13 * norm
    assert abs(r.theta - theta_star) < 6 * r.se_theta
    assert abs(r.twologlik - 2.0 * ll) <= len(y) * EPS * abs(ll) and r.fit.loglik == r.twologlik / 2.0


def test_poisson_limit():
    """theta = 1e12: V = mu (1 + mu / theta) and the deviance rows equal the Poisson's up to what the formulas'
    own rounding allows.  log((y + theta) / (mu + theta)) is the log of a number within 1e-11 of 1 that carries a
    relative rounding of eps, so each deviance row has an absolute error ~ theta * eps = 2e-4 -- random in sign,
    so the sum over n rows wanders by ~ sqrt(n) * theta * eps.  The coefficients feel it only through the stop
    rule; they are compared at the bar the weights' perturbation mu / theta = 1e-11 sets (times cond)."""
    theta = 1e12
    X, y, off, pw, _ = NB.make_case("log", 3001, 6, 2.0, 6)
    tol = 1e-1   # well above the deviance's rounding at this theta (below), far below the first steps
    a = NB.fit_glm(X, y, theta, "log", offset=off, prior=pw, tol=tol)
    b = LR.fit_glm(X, y, "poisson", "log", offset=off, prior=pw, tol=tol)
    dev_bar = 8 * np.sqrt(len(y)) * theta * EPS * 2.0
    cerr = np.max(np.abs(a.coefs - b.coefs) / np.abs(b.coefs))
    print(f"\npoisson limit: iterations {a.iter} / {b.iter}, |dev diff| {abs(a.deviance - b.deviance):.3g} "
          f"(bar {dev_bar:.3g}), coef rel err {cerr:.2e}")
    assert a.iter == b.iter
    assert abs(a.deviance - b.deviance) < dev_bar
    cond = LR.gram_cond(X, b, "poisson", "log", pw)
    assert cerr < 1e3 * cond * (b.mu.max() / theta + EPS)
    assert np.max(np.abs(a.stderr - b.stderr) / b.stderr) < 1e3 * cond * (b.mu.max() / theta + EPS)


def test_warm_start_from_the_fit_stops_at_once():
    X, y, off, pw, _ = NB.make_case("log", 2001, 5, 2.0, 7)
    f = NB.fit_glm(X, y, 2.0, "log", offset=off, prior=pw, tol=1e-10)
    g = NB.fit_glm(X, y, 2.0, "log", start=f.coefs, offset=off, prior=pw, tol=1e-6)
    assert g.iter == 1 and g.null_deviance == f.null_deviance
    assert abs(g.dev_trace[0] - f.deviance) < 1e-9 * f.deviance
    p = NB.fit_start(X, y, "poisson", "log", f.coefs, offset=off, prior=pw, tol=1e-8)
    q = LR.fit_glm(X, y, "poisson", "log", offset=off, prior=pw, tol=1e-8)
    assert np.max(np.abs(p.coefs - q.coefs) / np.abs(q.coefs)) < 1e-8 and p.null_deviance == q.null_deviance
