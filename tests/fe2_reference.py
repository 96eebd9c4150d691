"""numpy reference of the two-way fixed-effects GLM (sglm_fit_glm_fe2 / sglm_fe2_pass / sglm_vcov_fe2), built by
other routes than the engine's.

TEST INFRASTRUCTURE ONLY (a plain helper module of tests/test_fe2_reference.py, tests/test_fe2_api.py and
tests/test_gpu_fe2.py).  It imports tests/fe_reference.py for the rows and the one-way pieces.

  components   union-find over the G + H levels in plain Python (the engine: sglm_fe2_plan)
  dummy design [X | D1 | D2 without one column per component (its lowest factor-2 code) and without the columns
               of codes that have no rows]; dummy_fit2 is the dummy-variable IRLS on it
  sweeps       the block Gauss-Seidel sweeps of the engine restated with np.add.at, the same stop rule: the
               largest over the columns of max |change| / max |Y| (over both factors) <= tol
  demeaned     the rows of [X | z] projected off the dummy columns: by lstsq on sqrt(w) D (fp64, dense), or by
               alternating projections on the rows in np.longdouble run to 1e-19 -- A, b are their Gram
  meat         S_g = sum_{i in g} u_i x~_i of the explicitly demeaned rows x~

Factor-2 patterns (factor 1 is fe_reference.make_ids):
  cycle     i % 7 (the balanced panel)      random    uniform over 9 codes
  two_comp  two components: the lower half of factor 1's levels meets codes 0..2, the upper half 3..5
  nested    h = g % 4, a function of g: G_eff + H_eff - ncomp = G_eff
  giant     3 codes, 98 % of the rows in code 1      empty   8 codes, code 5 without rows      single   H = 1
"""
import numpy as np

import fe_reference as FR

PATTERNS2 = ("cycle", "random", "two_comp", "nested", "giant", "empty", "single")


def make_ids2(pattern, ids1, G, seed=77):
    n = len(ids1)
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    if pattern == "cycle":
        ids, H = i % 7, 7
    elif pattern == "random":
        ids, H = rng.integers(0, 9, n), 9
    elif pattern == "two_comp":
        ids, H = np.where(ids1 < G // 2, rng.integers(0, 3, n), 3 + rng.integers(0, 3, n)), 6
    elif pattern == "nested":
        ids, H = ids1 % 4, 4
    elif pattern == "giant":
        ids, H = rng.choice(3, size=n, p=[0.01, 0.98, 0.01]), 3
    elif pattern == "empty":
        ids, H = rng.integers(0, 7, n), 8
        ids = np.where(ids >= 5, ids + 1, ids)
    elif pattern == "single":
        ids, H = np.zeros(n, dtype=np.int64), 1
    else:
        raise ValueError(pattern)
    return ids.astype(np.int64), H


def components(ids1, ids2, G, H):
    """(comp1 [G], comp2 [H], low [ncomp]): the component of every level (-1: no rows), numbered by their
    lowest factor-2 code, and that code."""
    par = list(range(G + H))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    for g, h in set(zip(ids1.tolist(), ids2.tolist())):
        a, b = find(g), find(G + h)
        if a != b:
            par[max(a, b)] = min(a, b)
    comp1, comp2, low, of_root = np.full(G, -1), np.full(H, -1), [], {}
    for h in sorted(set(ids2.tolist())):
        r = find(G + h)
        if r not in of_root:
            of_root[r] = len(low)
            low.append(h)
        comp2[h] = of_root[r]
    for g in set(ids1.tolist()):
        comp1[g] = of_root[find(g)]
    return comp1, comp2, np.array(low, dtype=np.int64)


def dummies(ids, L):
    D = np.zeros((len(ids), L))
    D[np.arange(len(ids)), ids] = 1.0
    return D


def dummy_design2(X, ids1, ids2, G, H):
    """([X | D1 | D2 kept], kept): kept = the factor-2 codes with rows that are not a component's lowest."""
    _, comp2, low = components(ids1, ids2, G, H)
    kept = np.array([h for h in range(H) if comp2[h] >= 0 and h not in set(low.tolist())], dtype=np.int64)
    return np.asfortranarray(np.hstack([X, dummies(ids1, G), dummies(ids2, H)[:, kept]])), kept


def split_coefs(coefs, p, G, H, ids2, kept):
    """(beta, alpha, gamma) of a dummy fit: gamma 0 at the components' lowest codes, NaN at codes without rows."""
    gamma = np.where(np.bincount(ids2, minlength=H) > 0, 0.0, np.nan)
    gamma[kept] = coefs[p + G:]
    return coefs[:p], coefs[p:p + G], gamma


def dummy_fit2(X, y, ids1, ids2, G, H, fam, lnk, m=None, off=None, pw=None, theta=None, tol=1e-6, npart=1, max_iter=0):
    """The dummy-variable IRLS on dummy_design2: (fit, kept)."""
    import links_reference as LR
    import negbin_reference as NB
    import pyoracle as po
    XD, kept = dummy_design2(X, ids1, ids2, G, H)
    if fam == "negbin":
        return NB.fit_glm(XD, y, theta, lnk, offset=off, prior=pw, tol=tol, npart=npart, max_iter=max_iter), kept
    if fam in po.FAMILIES and lnk in po.LINKS and (fam == "binomial" or LR.CANONICAL[fam] == lnk):
        return po.fit_glm(XD, y, fam, lnk, m=m, offset=off, prior=pw, tol=tol, npart=npart, max_iter=max_iter), kept
    return LR.fit_glm(XD, y, fam, lnk, m=m, offset=off, prior=pw, tol=tol, npart=npart, max_iter=max_iter), kept


def rows2(X, y, beta, alpha, gamma, ids1, ids2, fam, lnk, m=None, off=None, pw=None, theta=None, mode=0, mu0=None):
    """(w, z, u) at (beta, alpha, gamma): fe_reference.rows with gamma_h in the offset."""
    n = len(y)
    o2 = (np.zeros(n) if off is None else off) + (0.0 if gamma is None else np.nan_to_num(gamma)[ids2])
    return FR.rows(X, y, beta, alpha, ids1, fam, lnk, m=m, off=o2, pw=pw, theta=theta, mode=mode, mu0=mu0)


def level_sums(M, w, ids, L):
    S, W = np.zeros((L, M.shape[1])), np.zeros(L)
    np.add.at(S, ids, w[:, None] * M)
    np.add.at(W, ids, w)
    return S, W


def pinned(ids1, ids2, G, H):
    """Factor-2 codes whose c stays 0: no rows, or the only factor-2 level of their component."""
    _, comp2, low = components(ids1, ids2, G, H)
    count = np.bincount(comp2[comp2 >= 0], minlength=len(low))
    return np.array([comp2[h] < 0 or count[comp2[h]] == 1 for h in range(H)])


def sweeps(M, w, ids1, ids2, G, H, tol=1e-12, max_sweeps=10000, Y0=None):
    """(a [G x k], c [H x k], sweeps): block Gauss-Seidel on K Y = S from Y0 (zeros), the engine's stop rule."""
    S1, W1 = level_sums(M, w, ids1, G)
    S2, W2 = level_sums(M, w, ids2, H)
    pin = pinned(ids1, ids2, G, H)
    a, c = (np.zeros_like(S1), np.zeros_like(S2)) if Y0 is None else (Y0[0].copy(), Y0[1].copy())
    ok1, ok2 = W1 > 0, (W2 > 0) & ~pin
    for k in range(1, max_sweeps + 1):
        T1 = np.zeros_like(S1)
        np.add.at(T1, ids1, w[:, None] * c[ids2])
        a1 = np.where(ok1[:, None], (S1 - T1) / np.where(ok1, W1, 1.0)[:, None], 0.0)
        if pin.all():
            return a1, c, k
        T2 = np.zeros_like(S2)
        np.add.at(T2, ids2, w[:, None] * a1[ids1])
        c1 = np.where(ok2[:, None], (S2 - T2) / np.where(ok2, W2, 1.0)[:, None], 0.0)
        d = np.maximum(np.abs(a1 - a).max(axis=0), np.abs(c1 - c).max(axis=0))
        mag = np.maximum(np.abs(a1).max(axis=0), np.abs(c1).max(axis=0))
        a, c = a1, c1
        change = float(np.max(np.where(d == 0.0, 0.0, d / np.where(mag == 0.0, 1.0, mag))))
        if change <= tol:
            return a, c, k
    raise RuntimeError(f"no convergence after {max_sweeps} sweeps: {change}")


def downdate(X, z, w, ids1, ids2, G, H, tol=1e-12):
    """dict(A, b, a, c, sweeps, S1, W1, S2, W2, XtWX): the engine's route -- X'W[X | z] - S_X' Y, X block symmetrised."""
    p = X.shape[1]
    M = np.column_stack([X, z])
    a, c, k = sweeps(M, w, ids1, ids2, G, H, tol)
    S1, W1 = level_sums(M, w, ids1, G)
    S2, W2 = level_sums(M, w, ids2, H)
    full = X.T @ (w[:, None] * M)
    D = S1[:, :p].T @ a + S2[:, :p].T @ c
    G0 = np.tril(full[:, :p]) + np.tril(full[:, :p], -1).T  # the engine's X'WX is a packed triangle
    A = G0 - 0.5 * (D[:, :p] + D[:, :p].T)
    return dict(A=A, b=full[:, p] - D[:, p], a=a, c=c, sweeps=k, S1=S1, W1=W1, S2=S2, W2=W2, XtWX=full[:, :p])


def demean_lstsq(M, w, ids1, ids2, G, H):
    """The rows of M projected off [D1 | D2] in the w inner product (fp64, dense, minimum-norm lstsq)."""
    D = np.hstack([dummies(ids1, G), dummies(ids2, H)])
    sw = np.sqrt(w)
    coef = np.linalg.lstsq(sw[:, None] * D, sw[:, None] * M, rcond=None)[0]
    return M - D @ coef


def demean_map(M, w, ids1, ids2, G, H, dtype=np.longdouble, tol=1e-19, max_iter=20000):
    """The same projection by alternating projections on the rows themselves, in `dtype`, run to `tol`."""
    R = M.astype(dtype)
    wd = w.astype(dtype)
    D1, D2 = dummies(ids1, G).astype(dtype), dummies(ids2, H).astype(dtype)
    W1, W2 = D1.T @ wd, D2.T @ wd
    i1, i2 = np.where(W1 > 0, 1 / np.where(W1 > 0, W1, 1), 0)[:, None], np.where(W2 > 0, 1 / np.where(W2 > 0, W2, 1), 0)[:, None]
    scale = np.abs(R).max(axis=0)
    for _ in range(max_iter):
        m1 = (D1.T @ (wd[:, None] * R)) * i1
        R = R - m1[ids1]
        m2 = (D2.T @ (wd[:, None] * R)) * i2
        R = R - m2[ids2]
        if float(np.max(np.maximum(np.abs(m1).max(axis=0), np.abs(m2).max(axis=0)) / scale)) <= tol:
            return R
    raise RuntimeError("alternating projections did not converge")


def gram_of(R, w, p):
    """(A, b) of demeaned rows R = [X~ | z~]."""
    wd = w.astype(R.dtype)
    A = R[:, :p].T @ (wd[:, None] * R[:, :p])
    b = R[:, :p].T @ (wd * R[:, p])
    return A.astype(np.float64), b.astype(np.float64)


def fe2_pass(X, y, beta, alpha, gamma, ids1, ids2, G, H, fam, lnk, **kw):
    """One concentrated step at (beta, alpha, gamma) by the lstsq route: dict(A, b, S1, W1, S2, W2, Y0, XtWX, w, z),
    S with the z column last; Y0 one solution of K Y = S (the minimum-norm one)."""
    p = X.shape[1]
    w, z, _ = rows2(X, y, beta, alpha, gamma, ids1, ids2, fam, lnk, **kw)
    M = np.column_stack([X, z])
    R = demean_lstsq(M, w, ids1, ids2, G, H)
    A, b = gram_of(R, w, p)
    S1, W1 = level_sums(M, w, ids1, G)
    S2, W2 = level_sums(M, w, ids2, H)
    return dict(A=A, b=b, S1=S1, W1=W1, S2=S2, W2=W2, XtWX=X.T @ (w[:, None] * X), w=w, z=z, M=M)


def remove_shift(Y, ids1, ids2, G, H):
    """Y [(G + H) x k] with its per-component null-space part taken out: within a component, c of the lowest
    factor-2 code becomes 0 (a moves the other way); levels without rows are left as they are."""
    comp1, comp2, low = components(ids1, ids2, G, H)
    Y = Y.copy()
    a, c = Y[:G], Y[G:]
    for k, h0 in enumerate(low):
        shift = c[h0].copy()
        c[comp2 == k] -= shift
        a[comp1 == k] += shift
    return Y


def normalise(alpha, gamma, ids1, ids2, G, H):
    """(alpha, gamma) shifted within every component so that gamma of its lowest factor-2 code is 0."""
    comp1, comp2, low = components(ids1, ids2, G, H)
    shift = np.nan_to_num(gamma)[low]
    return (alpha + np.where(comp1 >= 0, shift[comp1], 0.0), gamma - np.where(comp2 >= 0, shift[comp2], 0.0))


def solve_K(M, w, ids1, ids2, G, H):
    """A solution Y [(G + H) x k] of K Y = S by dense lstsq (for comparisons after remove_shift)."""
    D = np.hstack([dummies(ids1, G), dummies(ids2, H)])
    sw = np.sqrt(w)
    return np.linalg.lstsq(sw[:, None] * D, sw[:, None] * M, rcond=None)[0]


def meat2(X, u, w, ids1, ids2, G, H):
    """M = S'S, S_g = sum_{i in g} u_i x~_i over the explicitly demeaned rows."""
    Xt = demean_lstsq(X, w, ids1, ids2, G, H)
    S = np.zeros((G, X.shape[1]))
    np.add.at(S, ids1, u[:, None] * Xt)
    return S.T @ S


def dummy_cov2(X, y, beta, alpha, gamma, ids1, ids2, G, H, fam, lnk, type="HC1", cadjust=True, m=None, off=None, pw=None):
    """(V, C): the beta block of cluster_reference.cluster_cov (clustered on factor 1) on dummy_design2 at
    (beta, alpha, gamma): its regressor count is p + G + H_rows - ncomp."""
    import cluster_reference as CR
    p = X.shape[1]
    XD, kept = dummy_design2(X, ids1, ids2, G, H)
    coef = np.concatenate([beta, np.nan_to_num(alpha), np.nan_to_num(gamma)[kept]])
    ref = CR.cluster_cov(XD, y, coef, fam, lnk, ids1, G, type, cadjust, m=m, off=off, pw=pw)
    return ref["V"][:p, :p], ref["C"][:p, :p]


def drop_uninformative(ids1, ids2, y, fam, m=None, prior=None):
    """The rows to keep, by brute force: drop the rows of every level (either factor) whose rows of positive
    weight all have y = 0 (or all y = m), again and again until no such level is left.  (keep [n] bool, rounds)"""
    n = len(y)
    keep = np.ones(n, dtype=bool)
    if fam not in ("poisson", "negbin", "binomial"):
        return keep, 0
    pos = np.ones(n, dtype=bool) if prior is None else np.asarray(prior) > 0
    rounds = 0
    while True:
        bad = np.zeros(n, dtype=bool)
        for ids in (ids1, ids2):
            for l in np.unique(ids[keep]):
                r = keep & (ids == l)
                rr = r & pos
                if not rr.any():
                    continue
                if np.all(y[rr] == 0) or (fam == "binomial" and np.all(y[rr] == (1.0 if m is None else m[rr]))):
                    bad |= r
        if not bad.any():
            return keep, rounds
        keep &= ~bad
        rounds += 1


def make_case2(fam, lnk, n, p, ids1, G, ids2, H, seed, theta=2.0, zero_weights=True):
    """dict(X, y, m, off, pw, beta, alpha, gamma): fe_reference.make_case's design with y drawn from the two-way
    model; every family with an offset and prior weights, a few of them exactly 0 (zero_weights)."""
    import np_reference as R
    from sparkglm_amd import synth
    rng = np.random.default_rng(2000 + seed)
    X = np.array(synth.generate(0, 0, n, p + 1, seed)[0][:, 1:])
    sd = 1.0 / np.sqrt(3.0 * (p + 1))
    X = np.asfortranarray(X + (rng.normal(size=(G, p)) * sd)[ids1] + (rng.normal(size=(H, p)) * sd)[ids2])
    beta = synth.beta_star(p + 1, 0)[1:]
    alpha, gamma = rng.normal(size=G) * 0.4, rng.normal(size=H) * 0.3
    off = rng.uniform(-0.1, 0.1, n)
    pw = 0.5 + rng.uniform(size=n)
    if zero_weights:
        pw[rng.choice(n, size=max(n // 50, 1), replace=False)] = 0.0
    lin = X @ beta + alpha[ids1] + gamma[ids2]
    m = None
    if fam == "binomial":
        m = rng.integers(5, 10, n).astype(np.float64)
        pr = np.clip(R.unlink("binomial", lnk, 0.7 * lin + off, 1.0), 0.05, 0.95)
        y = rng.binomial(m.astype(int), pr).astype(np.float64)
    elif fam in ("poisson", "negbin"):
        mu = np.exp(1.0 + 0.5 * lin + off)
        y = (rng.poisson(mu) if fam == "poisson" else rng.negative_binomial(theta, theta / (theta + mu))).astype(np.float64)
    elif fam == "gamma":
        y = rng.gamma(4.0, np.exp(0.5 * lin + off) / 4.0)
    else:
        y = lin + off + rng.normal(size=n)
    return dict(X=X, y=y, m=m, off=off, pw=pw, beta=beta, alpha=alpha, gamma=gamma)
