"""numpy reference of the cluster-robust covariance (sandwich::vcovCL), independent of the engine.

  u, C   tests/sandwich_reference.py (QR-based: the engine inverts the Gramian)
  S      np.add.at of the score rows u_i x_i into a G x p array    (the engine: segment sums + combine)
  M      S' S by BLAS                                              (the engine: its MFMA Gram pass)
  V      a C M C, symmetrised;  a = [HC1: (n - 1) / (n - p)] [cadjust: G / (G - 1)]

Error metric: sandwich_reference.scaled_err.

The id patterns of the tests live here too, with T = the engine's tile_rows (sglm_cluster_plan):
  singletons   arange(n): one segment per row
  sorted       run lengths 1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 T + 3, then runs of 37
  shuffled     the sorted ids under a seeded permutation
  interleaved  i % 37: every cluster has many one-row segments
  two_level    (i // 5) % 101
"""
import numpy as np

from sandwich_reference import sandwich, scaled_err  # noqa: F401  (scaled_err: the tests' metric)

PATTERNS = ("singletons", "sorted", "shuffled", "interleaved", "two_level")


def make_ids(pattern, n, T):
    """(ids int64 [n], G) of one pattern; an id the pattern never reaches below G does not occur."""
    i = np.arange(n)
    if pattern == "singletons":
        ids = i
    elif pattern == "interleaved":
        ids = i % 37
    elif pattern == "two_level":
        ids = (i // 5) % 101
    elif pattern in ("sorted", "shuffled"):
        runs = [1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
        ids = np.repeat(np.arange(len(runs)), runs)[:n]
        rest = n - len(ids)
        if rest > 0:
            ids = np.concatenate([ids, ids[-1] + 1 + np.arange(rest) // 37])
        if pattern == "shuffled":
            ids = ids[np.random.default_rng(12345).permutation(n)]
    else:
        raise ValueError(pattern)
    return ids.astype(np.int64), int(ids.max()) + 1


def segments(ids, T):
    """The segmentation rule restated: a new segment starts at row 0, where the id changes, and at
    every multiple of T.  (seg_start [nseg + 1], seg_cluster [nseg])"""
    ids = np.asarray(ids)
    n = len(ids)
    if n == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    i = np.arange(n)
    first = (i == 0) | (i % T == 0)
    first[1:] |= ids[1:] != ids[:-1]
    start = np.flatnonzero(first)
    return np.concatenate([start, [n]]).astype(np.int64), ids[start]


def adjustment(n, p, G, type, cadjust):
    a = (n - 1.0) / (n - p) if type == "HC1" else 1.0
    return a * (G / (G - 1.0)) if cadjust else a


def cluster_cov(X, y, beta, fam, lnk, ids, G, type="HC1", cadjust=True, m=None, off=None, pw=None, dtype=np.float64,
                reverse=False):
    """dict(V, M, S, C, u): the cluster-robust covariance at beta.  `dtype` / `reverse`: the sums of S
    and M in another precision or with the rows in reverse order (the reference's own error)."""
    n, p = X.shape
    ref = sandwich(X, y, beta, fam, lnk, "HC0", m=m, off=off, pw=pw)
    u = ref["u"] if pw is None else np.where(pw == 0.0, 0.0, ref["u"])
    rows = (u[:, None] * X).astype(dtype)
    ids = np.asarray(ids)
    if reverse:
        rows, ids = rows[::-1], ids[::-1]
    S = np.zeros((G, p), dtype=dtype)
    np.add.at(S, ids, rows)
    M = S.T @ S
    C = ref["C"].astype(dtype)
    V = C @ M @ C
    V = 0.5 * (V + V.T) * dtype(adjustment(n, p, G, type, cadjust))
    return dict(V=V.astype(np.float64), M=M.astype(np.float64), S=S, C=ref["C"], u=u)
