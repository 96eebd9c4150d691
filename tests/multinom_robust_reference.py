"""Plain numpy reference of the multinomial sandwich covariance V = C M C (x n / (n - q) for HC1), C = inv(H),
M = sum_i (r_i r_i') (x) x_i x_i', r_i = pw_i (e_{y_i} - pi_i), class-major.  r_y = pw sum_{l != y} pi_l: nothing
cancels as pi_y -> 1.  dtype=np.longdouble: H and M in long double (the reference's own error); the solve is float64."""
import numpy as np

import multinom_reference as M


def score_rows(X, y, B, pw=None, dtype=np.float64):
    """R [n, K - 1] without the cancellation, exact zeros on the rows of weight 0."""
    r = M.rows(X, y, B, pw, dtype)
    P, w, yc = r["P"], r["pw"], r["yc"]
    K = P.shape[1]
    R = -P[:, 1:] * w[:, None]
    for j in range(1, K):
        others = sum(P[:, l] for l in range(K) if l != j)
        R[:, j - 1] = np.where(yc == j, w * others, R[:, j - 1])
    return np.where((w == 0)[:, None], 0, R)


def robust(X, y, B, pw=None, type="HC0", dtype=np.float64):
    """dict(meat, scale, H, cov): scale = sum_i |r_j r_k| |x x'|, what a cancelling meat is judged against."""
    Xd = X.astype(dtype)
    n, p = X.shape
    R = score_rows(X, y, B, pw, dtype)
    q = R.shape[1] * p
    meat, scale = np.zeros((q, q), dtype=dtype), np.zeros((q, q), dtype=dtype)
    for j in range(R.shape[1]):
        for k in range(j, R.shape[1]):
            om = R[:, j] * R[:, k]
            blk = Xd.T @ (om[:, None] * Xd)
            sc = np.abs(Xd).T @ (np.abs(om)[:, None] * np.abs(Xd))
            for A, b in ((meat, blk), (scale, sc)):
                A[j * p:(j + 1) * p, k * p:(k + 1) * p] = b
                A[k * p:(k + 1) * p, j * p:(j + 1) * p] = b.T
    H = M.multinom_pass(X, y, B, pw, dtype=dtype)["H"]
    f64 = lambda A: np.asarray(A, dtype=np.float64)
    out = dict(meat=f64(meat), scale=f64(scale), H=f64(H))
    C = np.linalg.inv(out["H"])
    V = C @ out["meat"] @ C
    out["cov"] = 0.5 * (V + V.T) * (n / (n - q) if type == "HC1" else 1.0)
    return out
