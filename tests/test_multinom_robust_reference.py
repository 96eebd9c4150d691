"""tests/multinom_robust_reference.py against np.longdouble (its own error) and against the per-row Kronecker
products it stands for.  No GPU.  Measured at 1300 x 20, K = 4: meat 3.1e-16, H 3.2e-16 (scaled), V 1.5e-15 -- the
1e-9 bars of tests/test_gpu_multinom_robust.py keep > 1e5 of margin from the reference alone."""
import numpy as np

import multinom_reference as M
import multinom_robust_reference as RR
from sandwich_reference import scaled_err


def test_own_error_against_longdouble():
    c = M.make_case(1300, 20, 4, 1)
    B = 0.8 * c["B"]
    for type in ("HC0", "HC1"):
        a = RR.robust(c["X"], c["y"], B, c["pw"], type)
        b = RR.robust(c["X"], c["y"], B, c["pw"], type, dtype=np.longdouble)
        errs = {k: scaled_err(a[k], b[k]) for k in ("meat", "H", "cov")}
        print(f"\nreference's own error ({type}): " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs["meat"], errs["H"]) <= 1e-14 and errs["cov"] <= 1e-12, errs
    assert scaled_err(a["meat"].T, a["meat"]) <= 1e-14


def test_meat_is_the_sum_of_the_rows_kronecker_products():
    c = M.make_case(60, 5, 3, 1)
    B = 0.8 * c["B"]
    R = RR.score_rows(c["X"], c["y"], B, c["pw"])
    want = sum(np.kron(np.outer(r, r), np.outer(x, x)) for r, x in zip(R, c["X"]))
    assert scaled_err(RR.robust(c["X"], c["y"], B, c["pw"])["meat"], want) <= 1e-14
    plain = M.rows(c["X"], c["y"], B, c["pw"])["R"]  # pw (1[y = j] - pi): the same away from pi_y = 1
    assert np.max(np.abs(R - plain)) <= 1e-15 and np.all(R[c["pw"] == 0] == 0.0)
