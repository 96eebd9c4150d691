"""The numpy / scipy reference of the negative binomial family and of MASS::glm.nb's theta estimation.

TEST INFRASTRUCTURE ONLY (a plain helper module of tests/test_negbin_reference.py, tests/test_negbin_api.py
and tests/test_gpu_negbin.py).  The reference project has no negative binomial, so nothing outside can be
compared against: this module restates the engine's algorithm operation for operation on
links_reference.fit_glm's skeleton, and tests/test_negbin_reference.py pins it to the likelihood itself
(the beta score and the theta score vanish at its fits, its theta derivatives are the differences of its
own log-likelihood, and theta -> infinity gives the Poisson fit).

  V(mu) = mu + mu^2 / theta
  unit deviance = pw [y log(max(y, 1) / mu) - (y + theta) log((y + theta) / (mu + theta))], family factor 2
  log-likelihood row = lgamma(theta + y) - lgamma(theta) - lgamma(y + 1) + theta log theta
                       + y log(mu + (y == 0)) - (theta + y) log(theta + mu)          (R's dnbinom(y, theta, mu = mu))
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from scipy.special import digamma, gammaln, polygamma

import links_reference as LR
import np_reference as R

LINKS = ("log", "sqrt", "identity")
THETA_EPS = 2.0 ** -13  # .Machine$double.eps^0.25


def variance(mu, theta):
    return mu + (mu * mu) / theta


def dev_rows(y, mu, pw, theta):
    with np.errstate(divide="ignore", invalid="ignore"):
        return pw * ((y * np.log(np.maximum(y, 1.0) / mu)) - ((y + theta) * np.log((y + theta) / (mu + theta))))


def deviance(y, mu, pw, theta, G=1):
    tot = 0.0
    for a, b in R.parts(len(y), G):
        tot = tot + 2.0 * float(np.ones(b - a) @ dev_rows(y[a:b], mu[a:b], pw[a:b], theta))
    return tot


def loglik_rows(y, mu, theta):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (gammaln(theta + y) - gammaln(theta) - gammaln(y + 1.0) + theta * np.log(theta)
                + y * np.log(mu + (y == 0)) - (theta + y) * np.log(theta + mu))


def loglik(y, mu, pw, theta):
    return float(np.sum(pw * loglik_rows(y, mu, theta)))


@dataclass
class Fit(LR.Fit):
    theta: float = None


def fit_glm(X, y, theta, lnk="log", start=None, offset=None, prior=None, tol=1e-6, npart=1, max_iter=0) -> Fit:
    """links_reference.fit_glm for negative.binomial(theta).  start (R's start=): the iterations begin at
    eta = X start + offset instead of link(mean(y)); dev_trace[0] is then the deviance at `start`, the null
    deviance stays the one at mean(y), iter counts solves."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    one = np.ones(n)
    off = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    pw = np.ones(n) if prior is None else np.asarray(prior, dtype=np.float64)
    G = max(int(npart), 1)
    theta = float(theta)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ysum = 0.0
        for a, b in R.parts(n, G):
            ysum = ysum + float(np.sum(y[a:b]))
        mu = np.full(n, ysum / n)
        eta = LR.link("negbin", lnk, mu, one)
        dev = deviance(y, mu, pw, theta, G)
        null_dev, deltad, it = dev, 1.0, 0
        invalid = [int(np.sum(~LR.valid_rows("negbin", lnk, eta, mu)))]
        coefs, se = np.zeros(X.shape[1]), np.zeros(X.shape[1])
        first = True
        if start is not None:
            coefs = np.asarray(start, dtype=np.float64).copy()
            eta = (X @ coefs) + off
            mu = LR.unlink("negbin", lnk, eta, one)
            dev = deviance(y, mu, pw, theta, G)
            invalid = [int(np.sum(~LR.valid_rows("negbin", lnk, eta, mu)))]
            first = False
        trace = [dev]
        while abs(deltad) > tol:
            if max_iter and it >= max_iter:
                break
            # (the first step of a cold start: mu = mean(y) itself on one partition, unlink(link(mean(y))) on several)
            mz = mu if (G == 1 or not first) else LR.unlink("negbin", lnk, eta, one)
            first = False
            grad = LR.lprime("negbin", lnk, mz, one)
            w = pw * (1.0 / (variance(mz, theta) * grad ** 2))
            z = eta + ((y + (-1.0 * mz)) * grad) + (-1.0 * off)
            coefs, se = R.wls(X, z, w, G)
            eta = (X @ coefs) + off
            mu = LR.unlink("negbin", lnk, eta, one)
            dev_old, dev = dev, deviance(y, mu, pw, theta, G)
            deltad = dev - dev_old
            it += 1
            trace.append(dev)
            invalid.append(int(np.sum(~LR.valid_rows("negbin", lnk, eta, mu))))
        pear = 0.0
        for a, b in R.parts(n, G):
            r = y[a:b] + (-1.0 * mu[a:b])
            pear = pear + float(np.sum(pw[a:b] * r ** 2 / variance(mu[a:b], theta)))
        ll = loglik(y, mu, pw, theta)
    return Fit(coefs, se, dev, null_dev, pear, ll, it, np.array(trace), invalid, mu, eta, theta)


def fit_start(X, y, family, lnk, start, offset=None, prior=None, tol=1e-6, npart=1, max_iter=0):
    """The warm-started fit of another family (poisson ...): links_reference.fit_glm's loop from `start`."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    one = np.ones(n)
    off = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    pw = np.ones(n) if prior is None else np.asarray(prior, dtype=np.float64)
    G = max(int(npart), 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        null_dev = R.deviance(family, y, np.full(n, float(np.sum(y)) / n), one, pw, G)
        coefs = np.asarray(start, dtype=np.float64).copy()
        se = np.zeros(X.shape[1])
        eta = (X @ coefs) + off
        mu = LR.unlink(family, lnk, eta, one)
        dev = R.deviance(family, y, mu, one, pw, G)
        deltad, it, trace = 1.0, 0, [dev]
        while abs(deltad) > tol:
            if max_iter and it >= max_iter:
                break
            grad = LR.lprime(family, lnk, mu, one)
            w = pw * (1.0 / (R.variance(family, mu, one) * grad ** 2))
            z = eta + ((y + (-1.0 * mu)) * grad) + (-1.0 * off)
            coefs, se = R.wls(X, z, w, G)
            eta = (X @ coefs) + off
            mu = LR.unlink(family, lnk, eta, one)
            dev_old, dev = dev, R.deviance(family, y, mu, one, pw, G)
            deltad = dev - dev_old
            it += 1
            trace.append(dev)
        pear = float(np.sum(pw * (y - mu) ** 2 / R.variance(family, mu, one)))
        ll = R.loglik(family, y, mu, one, pw, dev)
    return LR.Fit(coefs, se, dev, null_dev, pear, ll, it, np.array(trace), [], mu, eta)


# ---- theta ----
def theta_terms(y, mu, pw, theta):
    """(score, info, loglik, sum w (y/mu - 1)^2, sum w, sum |score terms|) at theta: MASS::theta.ml's score and
    info, summed over the rows of positive prior weight.  The last entry is the norm the score is judged against:
    sum over rows of w times the sum of the absolute values of the bracket's five terms (the score itself cancels
    to zero at the optimum)."""
    y, mu, pw = (np.asarray(v, dtype=np.float64) for v in (y, mu, pw))
    k = pw != 0.0
    y, mu, pw = y[k], mu[k], pw[k]
    theta = float(theta)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = digamma(theta + y) - digamma(theta)
        t2 = np.log(theta) - np.log(theta + mu)
        t3 = 1.0 - (y + theta) / (mu + theta)
        score = float(np.sum(pw * (t1 + t2 + t3)))
        norm = float(np.sum(pw * (np.abs(digamma(theta + y)) + np.abs(digamma(theta)) + abs(np.log(theta)) + 1.0
                                  + np.abs(np.log(theta + mu)) + np.abs((y + theta) / (mu + theta)))))
        info = float(np.sum(pw * (-polygamma(1, theta + y) + polygamma(1, theta) - 1.0 / theta + 2.0 / (mu + theta)
                                  - (y + theta) / (mu + theta) ** 2)))
        ll = loglik(y, mu, pw, theta)
        mom = float(np.sum(pw * (y / mu - 1.0) ** 2))
    return score, info, ll, mom, float(np.sum(pw)), norm


@dataclass
class ThetaML:
    theta: float
    se: float
    iters: int
    warn: int
    dels: list = field(default_factory=list)   # every Newton step
    thetas: list = field(default_factory=list)


def theta_ml(y, mu, pw, limit=25, eps=THETA_EPS) -> ThetaML:
    """MASS::theta.ml: t0 = sum w / sum w (y/mu - 1)^2; it = 0; del = 1;
    while ((it <- it + 1) < limit && |del| > eps) { t0 = |t0|; del = score / info; t0 = t0 + del }.
    warn bit 0: it == limit ("iteration limit reached"); bit 1: t0 < 0 -> 0 ("estimate truncated at zero")."""
    limit = 25 if limit <= 0 else int(limit)
    eps = THETA_EPS if not eps > 0 else float(eps)
    _, _, _, mom, sw, _ = theta_terms(y, mu, pw, 1.0)
    t0 = sw / mom
    it, dl, info = 0, 1.0, float("nan")
    dels, thetas = [], []
    while True:
        it += 1
        if not (it < limit and abs(dl) > eps):
            break
        t0 = abs(t0)
        score, info, _, _, _, _ = theta_terms(y, mu, pw, t0)
        dl = score / info
        t0 = t0 + dl
        dels.append(dl)
        thetas.append(t0)
    warn = 0
    if t0 < 0:
        t0, warn = 0.0, warn | 2
    if it == limit:
        warn |= 1
    return ThetaML(t0, float(np.sqrt(1.0 / info)), it, warn, dels, thetas)


@dataclass
class GlmNB:
    fit: Fit                 # the last inner fit (null_deviance at the final theta, loglik = twologlik / 2)
    theta: float
    se_theta: float
    twologlik: float
    outer_iter: int
    converged: bool
    theta_warn: int
    fit0: LR.Fit = None
    inner_traces: list = field(default_factory=list)   # every inner fit's deviance trace (fit0's first)
    theta_runs: list = field(default_factory=list)     # every theta_ml call (ThetaML)
    outer_stop: list = field(default_factory=list)     # |Lm0 - Lm| / d1 + |del| as judged before each outer step


def glm_nb(X, y, lnk="log", offset=None, prior=None, tol=1e-6, npart=1, maxit=25, epsilon=1e-8, theta_limit=25,
           theta_eps=THETA_EPS, inner_max_iter=0) -> GlmNB:
    """MASS::glm.nb in the engine's terms (include/sglm.h sglm_fit_glm_nb)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    pw = np.ones(n) if prior is None else np.asarray(prior, dtype=np.float64)
    kw = dict(offset=offset, prior=prior, tol=tol, npart=npart, max_iter=inner_max_iter)
    fit0 = LR.fit_glm(X, y, "poisson", lnk, **kw)
    beta, mu = fit0.coefs, fit0.mu
    runs = [theta_ml(y, mu, pw, theta_limit, theta_eps)]
    theta = runs[-1].theta
    Lm = 2.0 * loglik(y, mu, pw, theta)
    d1 = np.sqrt(2.0 * max(1.0, n - p))
    dl, Lm0, it = 1.0, Lm + 2.0 * d1, 0
    traces, stops, fit = [fit0.dev_trace], [], None
    while True:
        it += 1
        stop = abs(Lm0 - Lm) / d1 + abs(dl)
        stops.append(stop)
        if not (it <= maxit and stop > epsilon):
            break
        fit = fit_glm(X, y, theta, lnk, start=beta, **kw)
        beta, mu = fit.coefs, fit.mu
        traces.append(fit.dev_trace)
        t0 = theta
        runs.append(theta_ml(y, mu, pw, theta_limit, theta_eps))
        theta = runs[-1].theta
        dl = t0 - theta
        Lm0, Lm = Lm, 2.0 * loglik(y, mu, pw, theta)
    if fit is not None:
        G = max(int(npart), 1)
        fit.null_deviance = deviance(y, np.full(n, float(np.sum(y)) / n), pw, theta, G)
        fit.loglik = Lm / 2.0
    return GlmNB(fit, theta, runs[-1].se, Lm, it - 1, it <= maxit, runs[-1].warn, fit0, traces, runs, stops)


# ---- the shared inputs of the negative binomial tests ----
def make_case(lnk, n, p, theta_star, seed):
    """X (intercept + columns scaled by 1 / sqrt(p)), y ~ Poisson(mu g) with g ~ Gamma(theta*, 1 / theta*), an
    offset uniform in +-0.05 and prior weights 0.5 + U.  |eta*| stays modest, so mu is in range for every link:
    log eta* in about [0.2, 1.8], sqrt eta* in [1, 2.2], identity eta* in [1.5, 4.5]."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1.0, 1.0, (n, p - 1)) / np.sqrt(p)
    X = np.asfortranarray(np.column_stack([np.ones(n), Z]))
    b = rng.uniform(-1.0, 1.0, p - 1)
    lin = Z @ b
    lin = lin / max(np.max(np.abs(lin)), 1e-300)          # in [-1, 1]
    if lnk == "log":
        eta = 1.0 + 0.8 * lin
    elif lnk == "sqrt":
        eta = 1.6 + 0.6 * lin
    else:
        eta = 3.0 + 1.5 * lin
    # the true coefficients: the intercept and the scaled slopes that give eta
    scale = {"log": 0.8, "sqrt": 0.6, "identity": 1.5}[lnk] / max(np.max(np.abs(Z @ b)), 1e-300)
    beta = np.concatenate([[{"log": 1.0, "sqrt": 1.6, "identity": 3.0}[lnk]], b * scale])
    offset = rng.uniform(-0.05, 0.05, n)
    mu = LR.unlink("negbin", lnk, eta + offset, 1.0)
    g = rng.gamma(theta_star, 1.0 / theta_star, n)
    y = rng.poisson(mu * g).astype(np.float64)
    prior = 0.5 + rng.uniform(size=n)
    return X, y, offset, prior, beta


# ---- clearance of the stopping decisions (links_reference's rule) ----
EPSILONS = (1e-8, 1e-7, 1e-9)
THETA_EPSS = (2.0 ** -13, 2.0 ** -11, 2.0 ** -15)


def threshold_clearance(values, thr):
    """min over the judged quantities of max(v / thr, thr / v): how far every decision `v <= thr` is from
    flipping (links_reference.clearance for a list of judged values)."""
    v = np.maximum(np.abs(np.asarray(values, dtype=np.float64)), 1e-300)
    return float(np.min(np.maximum(v / thr, thr / v))) if len(v) else np.inf


def theta_clearance(run: ThetaML, eps):
    """theta.ml judges |del| of every step it took (the initial del = 1 is never near eps)."""
    return threshold_clearance(run.dels, eps)
