"""numpy reference of the sandwich (HC0-HC3) covariance, independent of the engine's algorithm.

  w, mu, g'   oracle/np_reference's row functions (as tests/test_gpu_influence.py::reference); a
              non-canonical pair takes unlink / g' by its link (tests/links_reference.py)
  h           rowsum(Q^2), Q R = qr(sqrt(w) X)          (the engine multiplies rows by an explicit inverse)
  C           inv(R) inv(R)' from that QR's R factor    (the engine inverts the Gramian)
  M           X' diag(omega) X by BLAS                  (the engine's MFMA Gram kernels)
  V           C M C (x n / (n - p) for HC1)

Error metric everywhere: e = max_ij |A - A_ref|_ij / sqrt(A_ref,ii A_ref,jj).
"""
import numpy as np

import links_reference as LR
import np_reference as R

HC_POWER = {"HC0": 0, "HC1": 0, "HC2": 1, "HC3": 2}


def sandwich(X, y, beta, fam, lnk, type="HC3", m=None, off=None, pw=None):
    """dict(V, M, C, h, u, omega) of the design at beta."""
    n, p = X.shape
    m = np.ones(n) if m is None else m
    off = np.zeros(n) if off is None else off
    pw = np.ones(n) if pw is None else pw
    eta = X @ beta + off
    F = R if fam == "binomial" or LR.CANONICAL[fam] == lnk else LR
    mu = F.unlink(fam, lnk, eta, m)
    g = F.lprime(fam, lnk, mu, m)
    v = R.variance(fam, mu, m)
    w = pw / (v * g * g)
    u = w * (y - mu) * g
    Q, Rf = np.linalg.qr(np.sqrt(w)[:, None] * X)
    h = np.sum(Q * Q, axis=1)
    Ri = np.linalg.inv(Rf)
    C = Ri @ Ri.T
    k = HC_POWER[type]
    omega = np.where(pw == 0.0, 0.0, u * u / (1.0 - h) ** k)
    M = X.T @ (omega[:, None] * X)
    V = C @ M @ C
    V = 0.5 * (V + V.T)
    if type == "HC1":
        V = V * (n / (n - p))
    return dict(V=V, M=M, C=C, h=h, u=u, omega=omega)


def scaled_err(A, ref):
    """max_ij |A - ref|_ij / sqrt(ref_ii ref_jj)"""
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(A - ref) / np.outer(d, d)))


def h_amp(h, type):
    """k max_i h_i / (1 - h_i): the first-order amplification of the leverage's bar through (1 - h)^-k"""
    return HC_POWER[type] * float(np.max(h / (1.0 - h)))
