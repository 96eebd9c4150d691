"""numpy reference of Firth's bias-reduced fits (sglm_fit_glm_firth / sglm_firth_pass), built by another route
than the engine's.

TEST INFRASTRUCTURE ONLY (a plain helper module of tests/test_firth_reference.py, tests/test_firth_api.py and
tests/test_gpu_firth.py).

  w, u, r    the row functions of oracle/np_reference and tests/links_reference: w = pw / (V g'^2),
             u = w (y - mu) g', r = (d2mu / deta2) / (dmu / deta) by link (firth_ratio)
  C, h       dense np.linalg.inv(X'WX) and the explicit quadratic forms h_i = w_i x_i' C x_i (rowsum((X C) o X)), never
             a tiled product
  g*         X' (u + h r / 2), one matrix-vector product
  fit        the driver's loop: start at sglm_fit_glm's first iterate (the initial pass at mean(y), one solve),
             beta += C g*, stop with beta when |C g*|_1 < epsilon, a step whose |g*|_inf is not finite or grows is
             retried at half its length (at most max_halvings times, then it stands)

`dtype` / `reverse` (np.longdouble, the rows in reverse order) give the reference's own error; in longdouble the
inverse is an unpivoted elimination (X'WX is positive definite).
"""
import numpy as np

import fe_reference as FR
import np_reference as R
from sparkglm_amd import synth

PAIRS = [("binomial", "logit"), ("binomial", "probit"), ("binomial", "cloglog"),
         ("poisson", "log"), ("poisson", "identity"), ("poisson", "sqrt")]


def make_case(fam, lnk, n, p, seed, zeros=True):
    """dict(X, y, m, off, pw, beta): an intercept and columns 1.. of synth.generate; binomial counts with trials m,
    an offset and prior weights of which (zeros) about 3 % are 0."""
    rng = np.random.default_rng(4000 + seed)
    X = np.asfortranarray(synth.generate(0, 0, n, p, seed)[0]).copy(order="F")
    X[:, 0] = 1.0
    beta = np.array(synth.beta_star(p, 0))
    lin = X[:, 1:] @ beta[1:]
    off = rng.uniform(-0.1, 0.1, n)
    pw = 0.5 + rng.uniform(size=n)
    if zeros:
        pw[rng.uniform(size=n) < 0.03] = 0.0
    m = None
    if fam == "binomial":
        m = rng.integers(20, 40, n).astype(np.float64)
        pr = np.clip(R.unlink("binomial", lnk, 0.7 * lin + off, 1.0), 0.05, 0.95)
        y = rng.binomial(m.astype(int), pr).astype(np.float64)
    else:
        mu = {"log": np.exp(3.0 + 0.5 * lin + off), "sqrt": (6.0 + 0.3 * lin + off) ** 2,
              "identity": np.maximum(40.0 + 4.0 * lin + off, 10.0)}[lnk]
        y = rng.poisson(mu).astype(np.float64)
    return dict(X=X, y=y, m=m, off=off, pw=pw, beta=beta)


def firth_ratio(lnk, eta, mu, m):
    """r = d'/d, d = dmu/deta: the binomial's m cancels."""
    if lnk == "logit":
        return 1 - 2 * (mu / m)
    if lnk == "probit":
        return -eta
    if lnk == "cloglog":
        return 1 - np.exp(eta)
    if lnk == "log":
        return np.ones_like(eta)
    if lnk == "sqrt":
        return 1 / eta
    return np.zeros_like(eta)  # identity


def _full(n, m, off, pw):
    return (np.ones(n) if m is None else m, np.zeros(n) if off is None else off, np.ones(n) if pw is None else pw)


def rows(X, y, beta, fam, lnk, m=None, off=None, pw=None, dtype=np.float64):
    """dict(w, u, r, mu, eta) at beta; rows of prior weight 0 carry exact zeros in w and u."""
    n = len(y)
    m, o, pw = (a.astype(dtype) for a in _full(n, m, off, pw))
    F = FR._fns(fam, lnk)
    eta = X.astype(dtype) @ np.asarray(beta, dtype=dtype) + o
    mu = F.unlink(fam, lnk, eta, m)
    g = F.lprime(fam, lnk, mu, m)
    dead = pw == 0
    with np.errstate(all="ignore"):
        w = np.where(dead, 0, pw / (R.variance(fam, mu, m) * g * g))
        u = np.where(dead, 0, w * (y.astype(dtype) - mu) * g)
    return dict(w=w, u=u, r=firth_ratio(lnk, eta, mu, m), mu=mu, eta=eta)


def _inv(A, dtype):
    if dtype == np.float64:
        return np.linalg.inv(A)
    A = np.array(A, dtype=dtype)
    k = A.shape[0]
    B = np.eye(k, dtype=dtype)
    for i in range(k):  # unpivoted elimination: A is positive definite
        f = A[i + 1:, i] / A[i, i]
        A[i + 1:, i:] -= f[:, None] * A[i, i:][None, :]
        B[i + 1:] -= f[:, None] * B[i][None, :]
    for i in range(k - 1, -1, -1):
        B[i] = (B[i] - A[i, i + 1:] @ B[i + 1:]) / A[i, i]
    return B


def firth_pass(X, y, beta, fam, lnk, m=None, off=None, pw=None, dtype=np.float64, reverse=False):
    """dict(A, C, g, hat, sum_hat, logdet, deviance, v, scale): one Firth pass at beta.  scale [p] = sum_i |v_i|
    |x_ij|, what the cancelling sum g* is judged against at a converged beta."""
    o = slice(None, None, -1) if reverse else slice(None)
    r = rows(X, y, beta, fam, lnk, m, off, pw, dtype)
    Xd = X.astype(dtype)[o]
    w, u, rr = r["w"][o], r["u"][o], r["r"][o]
    A = Xd.T @ (w[:, None] * Xd)
    C = _inv(A, dtype)
    q = np.sum((Xd @ C) * Xd, axis=1)
    h = w * q
    with np.errstate(all="ignore"):
        v = np.where(w == 0, 0, u + h * rr / 2)
    g = Xd.T @ v
    mm, _, pww = _full(len(y), m, off, pw)
    out = dict(A=A, C=C, g=g, hat=h[o], sum_hat=np.sum(h), v=v[o], scale=np.abs(Xd).T @ np.abs(v))
    out = {k: np.asarray(a, dtype=np.float64) if dtype == np.float64 else a for k, a in out.items()}
    if dtype == np.float64:
        out["logdet"] = float(np.linalg.slogdet(A)[1])
        with np.errstate(all="ignore"):
            out["deviance"] = R.deviance(fam, y, np.asarray(r["mu"], dtype=np.float64), mm, pww, 1)
    return out


def start(X, y, fam, lnk, m=None, off=None, pw=None):
    """(sglm_fit_glm's first iterate, the null deviance): the initial pass at mu = mean(y), eta = link(mu) with
    the offset ignored, and one solve."""
    n = len(y)
    mm, o, pww = _full(n, m, off, pw)
    F = FR._fns(fam, lnk)
    mu = np.full(n, float(np.sum(y)) / n)
    eta = F.link(fam, lnk, mu, mm)
    g = F.lprime(fam, lnk, mu, mm)
    w = np.where(pww == 0, 0.0, pww / (R.variance(fam, mu, mm) * g * g))
    z = eta + (y - mu) * g - o
    A = X.T @ (w[:, None] * X)
    return np.linalg.solve(A, X.T @ (w * z)), R.deviance(fam, y, mu, mm, pww, 1)


def firth_fit(X, y, fam, lnk, m=None, off=None, pw=None, epsilon=1e-8, maxit=100, max_halvings=12, beta_start=None):
    """The driver's loop over firth_pass: dict(coefs, stderr, deviance, null_deviance, pearson, loglik, iter,
    converged, halvings, pen_deviance, logdet, score_inf, sum_hat, trace, A) -- trace [iter + 1]: |C g*|_1 at
    every accepted iterate, the start included; everything at the returned coefficients."""
    kw = dict(m=m, off=off, pw=pw)
    beta, null_dev = start(X, y, fam, lnk, **kw)
    if beta_start is not None:
        beta = np.array(beta_start, dtype=np.float64)
    ev = lambda b: firth_pass(X, y, b, fam, lnk, **kw)
    inf = lambda e: float(np.max(np.abs(e["g"]))) if np.all(np.isfinite(e["g"])) else np.inf
    cur = ev(beta)
    it = halvings = 0
    converged = False
    trace = []
    while True:
        delta = cur["C"] @ cur["g"]
        trace.append(float(np.sum(np.abs(delta))))
        if trace[-1] < epsilon:
            converged = True
            break
        if it >= maxit:
            break
        f, hv = 1.0, 0
        while True:
            trial = beta + f * delta
            nxt = ev(trial)
            if (np.isfinite(inf(nxt)) and inf(nxt) <= inf(cur)) or hv >= max_halvings:
                break
            f, hv, halvings = f * 0.5, hv + 1, halvings + 1
        beta, cur, it = trial, nxt, it + 1
    mm, o, pww = _full(len(y), m, off, pw)
    mu = FR._fns(fam, lnk).unlink(fam, lnk, X @ beta + o, mm)
    with np.errstate(all="ignore"):
        pear = float(np.sum(pww * (y - mu) ** 2 / R.variance(fam, mu, mm)))
        ll = R.loglik(fam, y, mu, mm, pww, cur["deviance"])
    return dict(coefs=beta, stderr=np.sqrt(np.diag(cur["C"])), deviance=cur["deviance"], null_deviance=null_dev,
                pearson=pear, loglik=ll, iter=it, converged=converged, halvings=halvings,
                pen_deviance=cur["deviance"] - cur["logdet"], logdet=cur["logdet"], score_inf=inf(cur),
                sum_hat=float(cur["sum_hat"]), trace=np.array(trace), A=cur["A"])


def clearance(trace, epsilon):
    """How far the stop rule |delta|_1 < epsilon stays from every step it judges (up to and including the first
    converged one): min over those of max(d / epsilon, epsilon / d)."""
    d = np.asarray(trace, dtype=np.float64)
    conv = np.nonzero(d < epsilon)[0]
    d = np.maximum(d[: conv[0] + 1] if len(conv) else d, 1e-300)
    return float(np.min(np.maximum(d / epsilon, epsilon / d)))


def pick_epsilon(trace, lo=1e-9, hi=1e-4):
    """The epsilon in [lo, hi] that a long trace is clearest of: the geometric mean of two consecutive steps."""
    d = np.asarray(trace, dtype=np.float64)
    cands = [float(np.sqrt(d[k] * d[k + 1])) for k in range(len(d) - 1) if d[k + 1] > 0.0]
    cands = [e for e in cands if lo <= e <= hi]
    return max(cands, key=lambda e: clearance(trace, e))


def ml_fit(X, y, fam, lnk, m=None, off=None, pw=None, iters=25):
    """Plain IRLS from the same start, `iters` steps without a stop rule: the coefficients after each."""
    beta, _ = start(X, y, fam, lnk, m, off, pw)
    out = [beta]
    for _ in range(iters):
        r = rows(X, y, beta, fam, lnk, m, off, pw)
        with np.errstate(all="ignore"):
            A = X.T @ (r["w"][:, None] * X)
            try:
                beta = beta + np.linalg.solve(A, X.T @ r["u"])
            except np.linalg.LinAlgError:
                beta = np.full_like(beta, np.inf)
        out.append(beta)
    return np.array(out)
