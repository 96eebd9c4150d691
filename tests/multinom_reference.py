"""numpy reference of the multinomial logit fits (sglm_fit_multinom / sglm_multinom_pass), built by another route
than the engine's: dense matrix products, no tiles, no per-workgroup partials.

TEST INFRASTRUCTURE ONLY (a plain helper module of tests/test_multinom_reference.py, tests/test_multinom_api.py and
tests/test_gpu_multinom.py).

  rows       eta_0 = 0, eta_j = x' beta_j; mx = max(0, eta_1, ...); E_j = exp(eta_j - mx); S = E_0 + E_1 + ...;
             pi_j = E_j / S; log pi_y = (eta_y - mx) - log S; R_ij = pw_i (1[y_i = j] - pi_ij), exact zeros at pw = 0
  pass       g = vec(X'R) class-major; H_jj = X' diag(pw pi_j sum_{l != j} pi_l) X, H_jk = -X' diag(pw pi_j pi_k) X;
             D = -2 sum pw log pi_y; the weighted class counts N_k; null deviance -2 sum N_k log(N_k / N)
  fit        Newton from B = 0: delta = solve(H, g); B + t delta at t = 1, 1/2, ... accepted when D_new - D_old <=
             epsilon (|D_new| + 0.1), abandoned after max_halvings; stop when |D_old - D_new| / (|D_new| + 0.1) <
             epsilon after an accepted step

`dtype` / `reverse` (np.longdouble, the rows in reverse order) give the reference's own error.
B is [p, K - 1]; the parameter vector is B.T.reshape(-1) (class-major).
"""
import numpy as np


def softmax0(eta):
    """[n, K] from eta [n, K - 1] with the baseline's 0 in front: (P, mx, S, e)."""
    e = np.concatenate([np.zeros((eta.shape[0], 1), dtype=eta.dtype), eta], axis=1)
    mx = np.max(e, axis=1)
    E = np.exp(e - mx[:, None])
    S = E[:, 0].copy()
    for j in range(1, E.shape[1]):
        S = S + E[:, j]
    return E / S[:, None], mx, S, e


def make_case(n, p, K, seed):
    """dict(X, y, pw, B): an intercept plus N(0, 1/4) columns, true coefficients of size 0.6 / sqrt(p), prior
    weights in {0, 1, 2, 3}; every class has rows of positive weight."""
    rng = np.random.default_rng(7000 + 131 * seed + 17 * K + p)
    X = np.asfortranarray(np.c_[np.ones(n), 0.5 * rng.standard_normal((n, p - 1))])
    B = rng.uniform(-1.0, 1.0, (p, K - 1)) * (0.6 / np.sqrt(p))
    P = softmax0(X @ B)[0]
    y = np.minimum((rng.uniform(size=n)[:, None] > np.cumsum(P, axis=1)).sum(axis=1), K - 1).astype(np.float64)
    pw = rng.integers(0, 4, n).astype(np.float64)
    for k in range(K):  # (tiny cases: every class present with weight)
        if not np.any((y == k) & (pw > 0)):
            y[k % n], pw[k % n] = k, 1.0
    return dict(X=X, y=y, pw=pw, B=B)


def rows(X, y, B, pw=None, dtype=np.float64):
    """dict(P [n, K], R [n, K - 1], logpy [n], eta [n, K - 1], yc) at B; rows of prior weight 0 carry exact zeros
    in R and their y is not looked at."""
    n = X.shape[0]
    pw = (np.ones(n) if pw is None else np.asarray(pw)).astype(dtype)
    B = np.asarray(B, dtype=dtype)
    K = B.shape[1] + 1
    eta = X.astype(dtype) @ B
    P, mx, S, e = softmax0(eta)
    yc = np.where(pw > 0, np.nan_to_num(np.asarray(y, dtype=np.float64)), 0).astype(np.int64)
    logpy = (e[np.arange(n), yc] - mx) - np.log(S)
    ind = (yc[:, None] == np.arange(1, K)[None, :]).astype(dtype)
    R = np.where((pw == 0)[:, None], 0, pw[:, None] * (ind - P[:, 1:]))
    return dict(P=P, R=R, logpy=logpy, eta=eta, yc=yc, pw=pw)


def multinom_pass(X, y, B, pw=None, dtype=np.float64, reverse=False):
    """dict(H [q, q], g [q], deviance, sum_w, counts [K], null_deviance, P [n, K], R, scale [q]) at B.  scale =
    sum_i |R_ij| |x_ic|: what the cancelling score is judged against at a converged B."""
    o = slice(None, None, -1) if reverse else slice(None)
    r = rows(X, y, B, pw, dtype)
    Xd = X.astype(dtype)[o]
    P, R, w, yc = r["P"][o], r["R"][o], r["pw"][o], r["yc"][o]
    p, K = X.shape[1], P.shape[1]
    q = (K - 1) * p
    H = np.zeros((q, q), dtype=dtype)
    for j in range(1, K):
        for k in range(j, K):
            if j == k:
                om = w * P[:, j] * sum(P[:, l] for l in range(K) if l != j)
                blk = Xd.T @ (om[:, None] * Xd)
            else:
                blk = -(Xd.T @ ((w * P[:, j] * P[:, k])[:, None] * Xd))
            H[(j - 1) * p:j * p, (k - 1) * p:k * p] = blk
            H[(k - 1) * p:k * p, (j - 1) * p:j * p] = blk.T
    g = (Xd.T @ R).T.reshape(-1)
    scale = (np.abs(Xd).T @ np.abs(R)).T.reshape(-1)
    live = w > 0
    dev = -2 * np.sum(np.where(live, w * r["logpy"][o], 0))
    counts = np.array([np.sum(np.where(live & (yc == k), w, 0)) for k in range(K)], dtype=dtype)
    N = np.sum(counts)
    with np.errstate(all="ignore"):
        null = -2 * np.sum(counts * np.log(counts / N))
    out = dict(H=H, g=g, deviance=dev, sum_w=N, counts=counts, null_deviance=null, P=r["P"], R=r["R"], scale=scale)
    if dtype == np.float64:
        out = {k: (float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)) for k, v in out.items()}
    return out


def multinom_fit(X, y, K, pw=None, epsilon=1e-8, max_iter=100, max_halvings=12, start=None):
    """The driver's loop over multinom_pass: dict(coefs [K - 1, p], stderr [K - 1, p], cov, deviance, null_deviance,
    loglik, aic, iter, halvings, converged, score_inf, counts, H, trace) -- trace: |D_old - D_new| / (|D_new| + 0.1)
    of every accepted step; everything at the returned coefficients."""
    p = X.shape[1]
    q = (K - 1) * p
    B = np.zeros((p, K - 1)) if start is None else np.array(start, dtype=np.float64).reshape(p, K - 1)
    cur = multinom_pass(X, y, B, pw)
    it = halvings = 0
    converged = False
    trace = []
    while it < max_iter:
        delta = np.linalg.solve(cur["H"], cur["g"]).reshape(K - 1, p).T
        d_old, t, accepted = cur["deviance"], 1.0, False
        for hv in range(max_halvings + 1):
            trial = B + t * delta
            d_new = multinom_pass(X, y, trial, pw)["deviance"]
            if d_new - d_old <= epsilon * (abs(d_new) + 0.1):
                accepted = True
                break
            if hv < max_halvings:
                t, halvings = t * 0.5, halvings + 1
        if not accepted:
            break
        B, it = trial, it + 1
        cur = multinom_pass(X, y, B, pw)
        trace.append(abs(d_old - d_new) / (abs(d_new) + 0.1))
        if trace[-1] < epsilon:
            converged = True
            break
    cov = np.linalg.inv(cur["H"])
    dev = cur["deviance"]
    return dict(coefs=B.T.copy(), stderr=np.sqrt(np.diag(cov)).reshape(K - 1, p), cov=cov, deviance=dev,
                null_deviance=cur["null_deviance"], loglik=-dev / 2, aic=dev + 2 * q, iter=it, halvings=halvings,
                converged=converged, score_inf=float(np.max(np.abs(cur["g"]))), counts=cur["counts"], H=cur["H"],
                trace=np.array(trace), B=B)


def clearance(trace, epsilon):
    """How far the stop rule (relative deviance change < epsilon) stays from every step it judges (up to and
    including the first converged one): min over those of max(d / epsilon, epsilon / d)."""
    d = np.asarray(trace, dtype=np.float64)
    conv = np.nonzero(d < epsilon)[0]
    d = np.maximum(d[: conv[0] + 1] if len(conv) else d, 1e-300)
    return float(np.min(np.maximum(d / epsilon, epsilon / d)))


def pick_epsilon(trace, lo=1e-9, hi=1e-4):
    """The epsilon in [lo, hi] that a long trace is clearest of: the geometric mean of two consecutive steps (a
    step of exactly 0 counts as 1e-17)."""
    d = np.maximum(np.asarray(trace, dtype=np.float64), 1e-17)
    cands = [float(np.sqrt(d[k] * d[k + 1])) for k in range(len(d) - 1)]
    cands = [min(max(e, lo), hi) for e in cands]
    return max(cands, key=lambda e: clearance(trace, e))
