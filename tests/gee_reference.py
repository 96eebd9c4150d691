"""numpy reference of the GEE fits with an exchangeable working correlation (sglm_fit_glm_gee / sglm_gee_pass /
sglm_vcov_gee), built by another route than the engine's.

TEST INFRASTRUCTURE ONLY (a plain helper module of tests/test_gee_reference.py, tests/test_gee_api.py and
tests/test_gpu_gee.py).

  d, z, e    the row functions of oracle/np_reference and tests/links_reference (negbin: negbin_reference):
             d = sqrt(w), z the working response without the offset, e = d (y - mu) g'(mu)
  s, t, ...  np.add.at of the rows into G x p and G arrays             (the engine: segment sums + combine)
  A, b       sum_g X~_g' solve(R_g, X~_g) and X~_g' solve(R_g, z~_g) with the explicit dense block
             R_g = (1 - rho) I + rho 11' over the cluster's rows of positive prior weight -- np.linalg.solve per
             cluster, never the closed form c_g = rho / (1 - rho + n_g rho) the engine downdates with (a cluster
             of more than DENSE_MAX rows: conjugate gradients on the matrix-free product R v, _cg)
  rho, phi   the moment estimates of the issue (statsmodels / gee, ddof p) from E_g, Q_g, n_g
  fit        the driver's loop (start at mean(y) with rho = 0, |delta deviance| <= tol) over those steps
  V          naive phi inv(A); robust inv(A) M inv(A), M = sum U_g U_g', U_g = X~_g' solve(R_g, e_g)

`dtype` / `reverse` (np.longdouble, the rows in reverse order) give the reference's own error; in longdouble the
per-cluster solve is an unpivoted elimination (R_g is positive definite over the valid range of rho).
"""
import numpy as np

import fe_reference as FR
import links_reference as LR
import negbin_reference as NB
import np_reference as R
from sparkglm_amd import synth


def make_case(fam, lnk, n, p, ids, G, seed, theta=2.0, tau=0.4):
    """dict(X, y, m, off, pw, beta, alpha): an intercept and columns 1.. of synth.generate, y drawn from the
    model with a cluster-level random shift alpha_g (sd tau) in the linear predictor."""
    rng = np.random.default_rng(2000 + seed)
    kind = 3 if (fam, lnk) == ("gamma", "inverse") else 0
    X = np.asfortranarray(synth.generate(kind, 0, n, p, seed)[0]).copy(order="F")
    X[:, 0] = 1.0
    beta = np.array(synth.beta_star(p, kind))
    alpha = rng.normal(size=G) * tau
    lin = X[:, 1:] @ beta[1:] + alpha[ids]
    m = off = pw = None
    if fam == "binomial":
        m = rng.integers(5, 10, n).astype(np.float64)
        pr = np.clip(R.unlink("binomial", lnk, 0.7 * lin, 1.0), 0.05, 0.95)
        y = rng.binomial(m.astype(int), pr).astype(np.float64)
    elif fam in ("poisson", "negbin"):
        off = rng.uniform(-0.1, 0.1, n)
        pw = 0.5 + rng.uniform(size=n)
        mu = (2.0 + 0.3 * lin) ** 2 if lnk == "sqrt" else np.exp(1.0 + 0.5 * lin + off)
        y = (rng.poisson(mu) if fam == "poisson" else rng.negative_binomial(theta, theta / (theta + mu))).astype(np.float64)
    elif fam == "gamma":
        mu = 1.0 / (1.0 + X[:, 1:] @ beta[1:] + np.abs(alpha)[ids]) if lnk == "inverse" else np.exp(0.5 * lin)
        y = rng.gamma(4.0, mu / 4.0)
    else:
        y = lin + rng.normal(size=n)
    return dict(X=X, y=y, m=m, off=off, pw=pw, beta=beta, alpha=alpha)


def rows(X, y, beta, fam, lnk, m=None, off=None, pw=None, theta=None, mode=0, mu0=None):
    """dict(w, d, z, e, mu, keep) at beta; mode 1 / 2: the initial pass at mu0 (single / multiple).  Rows of
    prior weight 0 carry exact zeros; keep marks the rows of positive prior weight."""
    n = len(y)
    m = np.ones(n) if m is None else m
    pw = np.ones(n) if pw is None else pw
    o = np.zeros(n) if off is None else off
    F = FR._fns(fam, lnk)
    if mode == 0:
        eta = X @ beta + o
        mu = F.unlink(fam, lnk, eta, m)
    else:
        eta = F.link(fam, lnk, np.full(n, float(mu0)), m)
        mu = np.full(n, float(mu0)) if mode == 1 else F.unlink(fam, lnk, eta, m)
    g = F.lprime(fam, lnk, mu, m)
    dead = pw == 0.0
    w = np.where(dead, 0.0, pw / (FR.variance(fam, mu, m, theta) * g * g))
    d = np.sqrt(w)
    z = np.where(dead, 0.0, eta + (y - mu) * g - o)
    e = np.where(dead, 0.0, d * (y - mu) * g)
    return dict(w=w, d=d, z=z, e=e, mu=mu, keep=pw > 0.0)


def _solve(Rg, B, dtype):
    if dtype == np.float64:
        return np.linalg.solve(Rg, B)
    A = np.array(Rg, dtype=dtype)
    B = np.array(B, dtype=dtype)
    k = A.shape[0]
    for i in range(k):  # unpivoted elimination: R_g is positive definite
        f = A[i + 1:, i] / A[i, i]
        A[i + 1:, i:] -= f[:, None] * A[i, i:][None, :]
        B[i + 1:] -= f[:, None] * B[i][None, :]
    for i in range(k - 1, -1, -1):
        B[i] = (B[i] - A[i, i + 1:] @ B[i + 1:]) / A[i, i]
    return B


def _cg(rho, B):
    """solve(R, B) for R = (1 - rho) I + rho 11' without forming it: conjugate gradients on the matrix-free
    product (R has two distinct eigenvalues, so two steps reach the solution; a few more polish it).  For the
    clusters too large for a dense block."""
    B = B.reshape(B.shape[0], -1)
    Xs, Rr = np.zeros_like(B), B.copy()
    Pd = Rr.copy()
    for _ in range(6):
        RP = (1.0 - rho) * Pd + rho * Pd.sum(axis=0)[None, :]
        rr, den = (Rr * Rr).sum(axis=0), (Pd * RP).sum(axis=0)
        a = np.where(den > 0, rr / np.where(den > 0, den, 1.0), 0.0)
        Xs += a * Pd
        Rr = Rr - a * RP
        rn = (Rr * Rr).sum(axis=0)
        Pd = Rr + np.where(rr > 0, rn / np.where(rr > 0, rr, 1.0), 0.0) * Pd
    return Xs


DENSE_MAX = 2048  # rows of the largest cluster solved with a dense block


def group_sums(X, r, ids, G, dtype=np.float64, reverse=False):
    """dict(s, t, n, E, Q) by np.add.at."""
    o = slice(None, None, -1) if reverse else slice(None)
    p = X.shape[1]
    s, t, n, E, Q = (np.zeros((G, p), dtype=dtype),) + tuple(np.zeros(G, dtype=dtype) for _ in range(4))
    d, z, e, Xd = r["d"].astype(dtype), r["z"].astype(dtype), r["e"].astype(dtype), X.astype(dtype)
    np.add.at(s, ids[o], (d[:, None] * Xd)[o])
    np.add.at(t, ids[o], (d * z)[o])
    np.add.at(n, ids[o], r["keep"].astype(dtype)[o])
    np.add.at(E, ids[o], e[o])
    np.add.at(Q, ids[o], (e * e)[o])
    return dict(s=s, t=t, n=n, E=E, Q=Q)


def moments(gs, dtype=np.float64):
    """[sum E_g^2, sum Q_g, sum n_g (n_g - 1) / 2, N, n_max]"""
    n = gs["n"]
    return np.array([np.sum(gs["E"] * gs["E"]), np.sum(gs["Q"]), np.sum(n * (n - 1)) / 2, np.sum(n), np.max(n)],
                    dtype=dtype)


def phi_of(mom, p):
    return mom[1] / (mom[3] - p)


def rho_of(mom, p):
    return ((mom[0] - mom[1]) / 2) / ((mom[2] - p) * phi_of(mom, p))


def _blocks(X, r, ids, G, rho, cols, dtype, reverse):
    """sum_g X~_g' solve(R_g, C_g) for every column block C in cols (functions of the cluster's row index)."""
    p = X.shape[1]
    out = [np.zeros((p,) + c(np.arange(1)).shape[1:], dtype=dtype) for c in cols]
    order = range(G - 1, -1, -1) if reverse else range(G)
    Xd = X.astype(dtype)
    for g in order:
        idx = np.flatnonzero((ids == g) & r["keep"])
        if reverse:
            idx = idx[::-1]
        k = len(idx)
        if k == 0:
            continue
        Xt = r["d"].astype(dtype)[idx, None] * Xd[idx]
        if k <= DENSE_MAX:
            Rg = (dtype(1) - dtype(rho)) * np.eye(k, dtype=dtype) + dtype(rho) * np.ones((k, k), dtype=dtype)
        for o, c in zip(out, cols):
            C = c(idx).astype(dtype)
            if k <= DENSE_MAX:
                sol = _solve(Rg, C.reshape(k, -1), dtype).reshape(C.shape)
            else:
                sol = _cg(float(rho), C.astype(np.float64)).reshape(C.shape)
            o += Xt.T @ sol
    return out


def gee_pass(X, y, beta, ids, G, fam, lnk, rho=None, corstr="exchangeable", dtype=np.float64, reverse=False, **kw):
    """dict(A, b, s, t, n, E, Q, moments, rho, phi, XtWX): one step at beta with the dense blocks.  rho None:
    estimated from the moments at beta; the initial modes (kw mode 1 / 2) and independence use rho = 0."""
    p = X.shape[1]
    r = rows(X, y, beta, fam, lnk, **kw)
    gs = group_sums(X, r, ids, G, dtype, reverse)
    mom = moments(gs, dtype)
    if kw.get("mode", 0) != 0 or corstr == "independence":
        rho_used = dtype(0)
    else:
        rho_used = rho_of(mom, p) if rho is None else dtype(rho)
    Xt = lambda idx: r["d"].astype(dtype)[idx, None] * X.astype(dtype)[idx]
    zt = lambda idx: (r["d"].astype(dtype) * r["z"].astype(dtype))[idx]
    A, b = _blocks(X, r, ids, G, rho_used, (Xt, zt), dtype, reverse)
    out = {k: np.asarray(v, dtype=np.float64) for k, v in gs.items()}
    out.update(A=A.astype(np.float64), b=b.astype(np.float64), moments=mom.astype(np.float64), rho=float(rho_used),
               phi=float(phi_of(mom, p)), XtWX=X.T @ (r["w"][:, None] * X))
    return out


def score(X, y, beta, ids, G, fam, lnk, rho, **kw):
    """(sum_g D_g' inv(V_g) (y_g - mu_g) up to phi, X'W|z|): the estimating equation and its scale."""
    r = rows(X, y, beta, fam, lnk, **kw)
    U, = _blocks(X, r, ids, G, rho, (lambda idx: r["e"][idx],), np.float64, False)
    return U, X.T @ (r["w"] * np.abs(r["z"]))


def gee_fit(X, y, ids, G, fam, lnk, rho=None, corstr="exchangeable", m=None, off=None, pw=None, theta=None, tol=1e-6,
            max_iter=0, mode=1):
    """The driver's loop over gee_pass: dict(coefs, stderr, dev_trace, iter, deviance, null_deviance, pearson,
    loglik, rho, phi, A, XtWX) -- rho and phi re-evaluated at the returned coefficients."""
    n, p = X.shape
    kw = dict(m=m, off=off, pw=pw, theta=theta)
    mm = np.ones(n) if m is None else m
    pww = np.ones(n) if pw is None else pw
    o = np.zeros(n) if off is None else off
    mu0 = float(np.sum(y)) / n
    F = FR._fns(fam, lnk)
    dev_of = lambda mu: (NB.deviance(y, mu, pww, theta) if fam == "negbin" else R.deviance(fam, y, mu, mm, pww, 1))
    mu = np.full(n, mu0)
    dev = dev_of(mu)
    null_dev, trace, deltad, it = dev, [dev], 1.0, 0
    beta, st, Ainv = np.zeros(p), None, np.zeros((p, p))
    while abs(deltad) > tol and not (max_iter and it >= max_iter):
        st = gee_pass(X, y, beta if it else None, ids, G, fam, lnk, rho=rho, corstr=corstr, mode=0 if it else mode,
                      mu0=mu0, **kw)
        Ainv = np.linalg.inv(st["A"])
        beta = np.linalg.solve(st["A"], st["b"])
        mu = F.unlink(fam, lnk, X @ beta + o, mm)
        dev_old, dev = dev, dev_of(mu)
        deltad = dev - dev_old
        it += 1
        trace.append(dev)
    pear = float(np.sum(pww * (y - mu) ** 2 / FR.variance(fam, mu, mm, theta)))
    ll = NB.loglik(y, mu, pww, theta) if fam == "negbin" else R.loglik(fam, y, mu, mm, pww, dev)
    end = gee_pass(X, y, beta, ids, G, fam, lnk, rho=rho, corstr=corstr, **kw)
    return dict(coefs=beta, stderr=np.sqrt(np.diag(Ainv)), dev_trace=np.array(trace), iter=it, deviance=dev,
                null_deviance=null_dev, pearson=pear, loglik=ll, rho=end["rho"], phi=end["phi"], A=end["A"],
                XtWX=end["XtWX"])


def gee_cov(X, y, beta, rho, ids, G, fam, lnk, robust=True, cadjust=False, corstr="exchangeable", dtype=np.float64,
            reverse=False, **kw):
    """dict(V, M, C, phi): the covariance of beta at (beta, rho)."""
    p = X.shape[1]
    rho = 0.0 if corstr == "independence" else rho
    r = rows(X, y, beta, fam, lnk, **kw)
    Xt = lambda idx: r["d"].astype(dtype)[idx, None] * X.astype(dtype)[idx]
    A, = _blocks(X, r, ids, G, rho, (Xt,), dtype, reverse)
    C = _solve(A, np.eye(p, dtype=dtype), dtype) if dtype != np.float64 else np.linalg.inv(A)
    phi = phi_of(moments(group_sums(X, r, ids, G, dtype, reverse), dtype), p)
    M = np.zeros((p, p), dtype=dtype)
    if robust:
        order = range(G - 1, -1, -1) if reverse else range(G)
        for g in order:
            one = np.where(ids == g, True, False)
            rg = dict(r, keep=r["keep"] & one)
            U, = _blocks(X, rg, ids, G, rho, (lambda idx: r["e"].astype(dtype)[idx],), dtype, reverse)
            M += np.outer(U, U)
        V = C @ M @ C
        V = (V + V.T) / 2 * dtype(G / (G - 1.0) if cadjust else 1.0)
    else:
        V = phi * C
    return dict(V=V.astype(np.float64), M=M.astype(np.float64), C=C.astype(np.float64), phi=float(phi))


def gls(X, y, ids, G, rho):
    """Dense GLS of y on X under the block-exchangeable correlation: (beta, inv(X' inv(R) X))."""
    n = len(y)
    Rm = np.where(ids[:, None] == ids[None, :], rho, 0.0)
    Rm[np.arange(n), np.arange(n)] = 1.0
    RiX = np.linalg.solve(Rm, X)
    A = X.T @ RiX
    return np.linalg.solve(A, RiX.T @ y), np.linalg.inv(A)
