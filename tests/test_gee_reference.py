"""tests/gee_reference.py against itself and against independent restatements, on the CPU: its own rounding error
(fp64 against np.longdouble and against the rows in reverse order), the size of the estimated correlation, and
the identities the GPU tests lean on (independence is the plain GLM; Gaussian / identity with a fixed rho is dense
GLS; the estimating equation vanishes at a converged fit)."""
import numpy as np
import pytest

import fe_reference as FR
import gee_reference as GR
import links_reference as LR
from conftest import nrel, rel
from sandwich_reference import scaled_err

T = 128  # the engine's tile_rows (tests/test_gee_api.py asserts it)
N, P, SEED = 1300, 20, 2
_cases = {}


def case(pat, fam="poisson", lnk="log"):
    key = (pat, fam, lnk)
    if key not in _cases:
        ids, G = FR.make_ids(pat, N, T)
        c = GR.make_case(fam, lnk, N, P, ids, G, SEED)
        _cases[key] = (c, ids, G, dict(m=c["m"], off=c["off"], pw=c["pw"]))
    return _cases[key]


@pytest.mark.parametrize("pat", FR.PATTERNS)
def test_reference_error_and_rho_range(pat):
    c, ids, G, kw = case(pat)
    beta = c["beta"] * 0.8
    a = GR.gee_pass(c["X"], c["y"], beta, ids, G, "poisson", "log", **kw)
    assert 0.1 <= a["rho"] <= 0.6, a["rho"]  # the downdate is never trivially small
    errs = {}
    for label, alt in (("longdouble", dict(dtype=np.longdouble)), ("reverse", dict(reverse=True))):
        b = GR.gee_pass(c["X"], c["y"], beta, ids, G, "poisson", "log", **alt, **kw)
        errs[label] = dict(A=scaled_err(a["A"], b["A"]), b=nrel(a["b"], b["b"]), mom=rel(a["moments"], b["moments"]),
                           s=nrel(a["s"], b["s"]), t=nrel(a["t"], b["t"]), E=nrel(a["E"], b["E"]), Q=nrel(a["Q"], b["Q"]))
        for robust in (True, False):
            va = GR.gee_cov(c["X"], c["y"], beta, a["rho"], ids, G, "poisson", "log", robust=robust, **kw)
            vb = GR.gee_cov(c["X"], c["y"], beta, a["rho"], ids, G, "poisson", "log", robust=robust, **alt, **kw)
            errs[label]["V robust" if robust else "V naive"] = scaled_err(va["V"], vb["V"])
    print(f"\nREFERENCE ERROR {pat} (rho {a['rho']:.3f}, G {G}): " +
          "; ".join(f"{k}: " + ", ".join(f"{q} {v:.1e}" for q, v in e.items()) for k, e in errs.items()))
    worst = max(max(e.values()) for e in errs.values())
    assert worst <= 1e-11, errs  # the 1e-9 bars of the GPU tests keep two decades from the reference alone


@pytest.mark.parametrize("pat", ("sorted", "interleaved"))
def test_negative_fixed_rho_keeps_the_reference_accurate(pat):
    c, ids, G, kw = case(pat)
    n_max = int(np.bincount(ids).max())
    rho = -0.5 / (n_max - 1)
    beta = c["beta"] * 0.8
    a = GR.gee_pass(c["X"], c["y"], beta, ids, G, "poisson", "log", rho=rho, **kw)
    b = GR.gee_pass(c["X"], c["y"], beta, ids, G, "poisson", "log", rho=rho, dtype=np.longdouble, **kw)
    err = max(scaled_err(a["A"], b["A"]), nrel(a["b"], b["b"]))
    print(f"\nREFERENCE ERROR negative rho {pat}: {err:.1e}")
    assert a["rho"] == rho and err <= 1e-11


def test_independence_is_the_plain_glm_iterate_by_iterate():
    c, ids, G, kw = case("two_level")
    o = LR.fit_glm(c["X"], c["y"], "poisson", "log", offset=kw["off"], prior=kw["pw"], tol=1e-8)
    f = GR.gee_fit(c["X"], c["y"], ids, G, "poisson", "log", corstr="independence", tol=1e-8, **kw)
    assert f["iter"] == o.iter and rel(f["dev_trace"], o.dev_trace) <= 1e-12
    assert rel(f["coefs"], o.coefs) <= 1e-10 and rel(f["stderr"], o.stderr) <= 1e-10 and f["rho"] == 0.0
    assert rel([f["pearson"], f["loglik"], f["null_deviance"]], [o.pearson, o.loglik, o.null_deviance]) <= 1e-12


def test_gaussian_identity_with_fixed_rho_is_dense_gls():
    c, ids, G, kw = case("sorted", "gaussian", "identity")
    beta, Ainv = GR.gls(c["X"], c["y"], ids, G, 0.3)
    f = GR.gee_fit(c["X"], c["y"], ids, G, "gaussian", "identity", rho=0.3, max_iter=2, **kw)
    # the first solve is the rho = 0 start (OLS), the second the GLS solve itself
    assert rel(f["coefs"], beta) <= 1e-9 and rel(f["stderr"], np.sqrt(np.diag(Ainv))) <= 1e-9
    g = GR.gee_fit(c["X"], c["y"], ids, G, "gaussian", "identity", rho=0.3, max_iter=3, **kw)
    assert rel(g["coefs"], f["coefs"]) <= 1e-12  # a fixed point: one GLS solve


@pytest.mark.parametrize("fam,lnk", (("poisson", "log"), ("binomial", "logit"), ("gamma", "log")))
def test_estimating_equation_vanishes_at_a_converged_fit(fam, lnk):
    c, ids, G, kw = case("two_level", fam, lnk)
    f = GR.gee_fit(c["X"], c["y"], ids, G, fam, lnk, tol=1e-10, **kw)
    # the last step used rho at the iterate before; at a fixed point the two agree
    U, scale = GR.score(c["X"], c["y"], f["coefs"], ids, G, fam, lnk, f["rho"], **kw)
    r = float(np.linalg.norm(U) / np.linalg.norm(scale))
    print(f"\nESTIMATING EQUATION {fam}/{lnk}: |U| / |X'W|z|| = {r:.2e} (rho {f['rho']:.3f}, phi {f['phi']:.3f}, "
          f"iter {f['iter']})")
    assert r <= 1e-4 and 0.0 < f["rho"] < 1.0
