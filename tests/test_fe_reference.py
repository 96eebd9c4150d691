"""tests/fe_reference.py against itself and against the project's other references, on the CPU: the
concentrated IRLS equals the dummy-variable IRLS (Frisch-Waugh-Lovell), its covariance equals the beta block
of cluster_reference.cluster_cov on [X | D], and the reference's own rounding error -- fp64 against
np.longdouble and against the rows in reverse order -- is asserted (and quoted by tests/test_gpu_fe.py)."""
import numpy as np
import pytest

import fe_reference as FR
from conftest import nrel, rel
from sandwich_reference import scaled_err

T = 128  # any tile works on the CPU; the GPU tests take the engine's


def case(fam="poisson", lnk="log", n=1300, p=5, pattern="sorted", seed=3):
    ids, G = FR.make_ids(pattern, n, T)
    c = FR.make_case(fam, lnk, n, p, ids, G, seed)
    return c, ids, G, dict(m=c["m"], off=c["off"], pw=c["pw"])


@pytest.mark.parametrize("pattern", FR.PATTERNS)
def test_patterns_are_small_factors(pattern):
    ids, G = FR.make_ids(pattern, 2 * T + 1000 + 15 * 6, T)
    assert 3 <= G <= 25 and set(np.unique(ids)) == set(range(G))


def test_concentrated_irls_is_the_dummy_irls():
    """Poisson / log, 1300 x 5, with offset and prior weights: the same iteration count and deviance trace,
    beta, the standard errors and alpha = the dummy coefficients."""
    c, ids, G, kw = case()
    o = FR.dummy_fit(c["X"], c["y"], ids, G, "poisson", "log", **kw)
    f = FR.fe_fit(c["X"], c["y"], ids, G, "poisson", "log", **kw)
    p = c["X"].shape[1]
    assert f["iter"] == o.iter and o.iter >= 3
    assert rel(f["trace"], o.dev_trace) < 1e-12
    assert rel(f["coefs"], o.coefs[:p]) < 1e-10 and rel(f["stderr"], o.stderr[:p]) < 1e-10
    assert rel(f["alpha"], o.coefs[p:]) < 1e-10


@pytest.mark.parametrize("fam,lnk", [("binomial", "logit"), ("gamma", "log"), ("gaussian", "identity"),
                                     ("negbin", "log"), ("poisson", "sqrt")])
def test_concentrated_irls_other_families(fam, lnk):
    c, ids, G, kw = case(fam, lnk, 900, 4, "two_level")
    th = dict(theta=2.0) if fam == "negbin" else {}
    o = FR.dummy_fit(c["X"], c["y"], ids, G, fam, lnk, **kw, **th)
    f = FR.fe_fit(c["X"], c["y"], ids, G, fam, lnk, **kw, **th)
    trace = getattr(o, "dev_trace", getattr(o, "trace", None))
    assert f["iter"] == o.iter
    assert rel(f["trace"], trace) < 1e-10
    assert rel(f["coefs"], o.coefs[:4]) < 1e-8 and rel(f["alpha"], o.coefs[4:]) < 1e-8


@pytest.mark.parametrize("t,ca", [("HC0", False), ("HC1", True)])
def test_covariance_is_the_beta_block_of_the_dummy_covariance(t, ca):
    """At a converged and at a perturbed (beta, alpha); without the U_g xbar_g term the perturbed point is
    off by far more than rounding."""
    c, ids, G, kw = case()
    f = FR.fe_fit(c["X"], c["y"], ids, G, "poisson", "log", **kw)
    for db, da in ((0.0, 0.0), (0.05, -0.03)):
        beta, alpha = f["coefs"] + db, f["alpha"] + da
        V = FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", t, ca, **kw)
        Vd, Cd = FR.dummy_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", t, ca, **kw)
        assert scaled_err(V["V"], Vd) < 1e-10 and scaled_err(V["C"], Cd) < 1e-10
        bad = FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", t, ca, correct=False, **kw)
        if db:
            assert scaled_err(bad["V"], Vd) > 1e-3


OWN = {}


@pytest.mark.parametrize("pattern", FR.PATTERNS)
def test_the_references_own_error(pattern):
    """fp64 against np.longdouble and against reversed row order at 1300 x 20, at a non-converged point: A,
    the group sums and V.  The GPU bars (1e-9) keep > 1e4 of margin from the reference alone."""
    c, ids, G, kw = case(n=1300, p=20, pattern=pattern)
    beta, alpha = c["beta"] * 0.8, c["alpha"] * 0.5
    base = FR.fe_pass(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", **kw)
    V = FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", **kw)["V"]
    worst = dict(A=0.0, S=0.0, t=0.0, W=0.0, V=0.0)
    for alt in (dict(dtype=np.longdouble), dict(reverse=True)):
        o = FR.fe_pass(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", **kw, **alt)
        worst["A"] = max(worst["A"], scaled_err(base["A"], o["A"]))
        for k in ("S", "t", "W"):
            worst[k] = max(worst[k], nrel(base[k], o[k]))
        worst["V"] = max(worst["V"], scaled_err(V, FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log",
                                                             **kw, **alt)["V"]))
    print(f"\nOWN ERROR {pattern}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["A"] <= 1e-13 and worst["V"] <= 1e-12
    assert max(worst["S"], worst["t"], worst["W"]) <= 1e-13
    cond = np.linalg.norm(base["XtWX"], 2) * np.linalg.norm(np.linalg.inv(base["A"]), 2)
    assert cond < 1e4  # the downdate keeps the parity bars' fixed 1e-9 on these designs


def test_zero_weight_group_and_uninformative_logic():
    from sparkglm_amd.glm import fe_codes, fe_drop_intercept, fe_offsets, fe_uninformative
    c, ids, G, kw = case(n=900, p=4, pattern="two_level")
    pw = kw["pw"].copy()
    pw[ids == 3] = 0.0
    f = FR.fe_fit(c["X"], c["y"], ids, G, "poisson", "log", m=None, off=kw["off"], pw=pw)
    assert np.isnan(f["alpha"][3]) and np.sum(np.isnan(f["alpha"])) == 1
    keep = ids != 3
    _, sub = np.unique(ids[keep], return_inverse=True)
    g = FR.fe_fit(c["X"][keep], c["y"][keep], sub, G - 1, "poisson", "log", off=kw["off"][keep], pw=pw[keep])
    assert rel(f["coefs"], g["coefs"]) < 1e-10 and f["iter"] == g["iter"]
    # the model layer's array logic
    labels = np.array([f"g{k:02d}" for k in ids])
    uniq, codes = fe_codes(labels)
    assert list(uniq) == sorted(set(labels)) and np.array_equal(uniq[codes], labels)
    Xi = np.column_stack([np.ones(len(ids)), c["X"]])
    X2, names = fe_drop_intercept(Xi, ["one", "a", "b", "c", "d"])
    assert names == ["a", "b", "c", "d"] and np.array_equal(X2, c["X"])
    y = c["y"].copy()
    y[ids == 5] = 0.0
    assert list(np.flatnonzero(fe_uninformative(ids, G, y, "poisson"))) == [5]
    assert not fe_uninformative(ids, G, y, "gaussian").any()
    pw2 = np.ones(len(y))
    pw2[ids == 5] = 0.0  # no row of positive weight: not uninformative, just empty
    assert not fe_uninformative(ids, G, y, "poisson", prior=pw2).any()
    mm = np.full(len(y), 4.0)
    yb = np.where(ids == 2, 4.0, np.where(ids == 7, 0.0, 2.0))
    assert list(np.flatnonzero(fe_uninformative(ids, G, yb, "binomial", m=mm))) == [2, 7]
    off = fe_offsets({"a": 1.0, "b": 2.0}, np.array(["b", "zz", "a"]), np.array([0.5, 0.5, 0.5]))
    assert off[0] == 2.5 and np.isnan(off[1]) and off[2] == 1.5
