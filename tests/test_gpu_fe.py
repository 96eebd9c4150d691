"""One-way fixed-effects GLM fits on the GPU (sglm_fit_glm_fe, sglm_fe_pass, sglm_vcov_fe: the kernels of fe.hip,
the segment-sum and combine kernels of cluster.hip, a Gram pass over the group sums) against
tests/fe_reference.py: the dummy-variable IRLS on [X | D] (Frisch-Waugh-Lovell: every iterate is the same) and
a numpy restatement of one concentrated step by another route (np.add.at, explicitly demeaned rows, QR).

Bars (the project's):
  fits    conftest.check_fit with cond = ||X'WX||_2 ||inv(A)||_2 -- the downdate A = X'WX - sum s s' / W loses
          that factor, not cond(A); alpha against the dummy coefficients within coef_bound at the dummy Gram's cond;
          dev_trace elementwise 1e-9; the iteration count where the oracle's trace is a factor 10 clear of tol
  A       scaled_err <= 1e-9;  b, s, t, W: nrel <= 1e-9 (the cluster tests' bars);  scalars rel <= 1e-9
  V       scaled_err <= 2 max(1e-9, K_BOUND cond eps), inv(A) alone half of that

The reference's own error, measured on the CPU (tests/test_fe_reference.py asserts it at 1300 x 20 for every id
pattern): fp64 against np.longdouble and against the rows in reverse order, A <= 3.6e-15, s / t / W <= 1.1e-15,
V <= 2.4e-14.  So the 1e-9 bars keep > 1e4 of margin from the reference alone.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import fe_reference as FR
import links_reference as LR
import np_reference as R
from conftest import K_BOUND, check_fit, coef_bound, nrel, rel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D
from sparkglm_amd.glm import fe_uninformative

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
T = L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0]  # the engine's tile_rows (no device)
SWEEP_P = (1, 5, 16, 17, 33, 64, 65, 129, 256)
SEED = 2  # every fit's oracle trace is a factor 10 clear of its tol at this seed (asserted per fit)


def v_bar(cond):
    return 2.0 * max(1e-9, K_BOUND * cond * EPS)


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def sweep_n(p):
    n = 2 * T + 1000 + 15 * (p % 7)
    assert n % T != 0  # the last tile is partial
    return n


_cases = {}


def case(fam, lnk, n, p, pattern, seed=SEED):
    """The data of one case and its kwargs for the references, made once per module."""
    key = (fam, lnk, n, p, pattern, seed)
    if key not in _cases:
        ids, G = FR.make_ids(pattern, n, T)
        c = FR.make_case(fam, lnk, n, p, ids, G, seed)
        assert not fe_uninformative(ids, G, c["y"], fam, c["m"], c["pw"]).any()
        kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
        if fam == "negbin":
            kw["theta"] = 2.0
        _cases[key] = (c, ids, G, kw)
    return _cases[key]


def load(e, c, ids, G, kw):
    if "theta" in kw:
        e.set_theta(kw["theta"])
    e.set_data(c["X"], c["y"], m=kw["m"], offset=kw["off"], prior=kw["pw"])
    e.set_clusters(ids, G)


def downdate_cond(ref):
    return float(np.linalg.norm(ref["XtWX"], 2) * np.linalg.norm(np.linalg.inv(ref["A"]), 2))


def check_pass(label, e, c, ids, G, kw, fam, lnk, beta, alpha, **mode):
    """fe_pass at (beta, alpha) against the reference's A, b, s, t, W and the pass's scalars."""
    refkw = {k: v for k, v in kw.items()}
    if beta is None:
        mu0 = float(np.sum(c["y"])) / len(c["y"])
        ref = FR.fe_pass(c["X"], c["y"], None, alpha, ids, G, fam, lnk, mode=mode.get("mode", 1), mu0=mu0, **refkw)
    else:
        ref = FR.fe_pass(c["X"], c["y"], beta, alpha, ids, G, fam, lnk, **refkw)
    A, b, S, t, W, s = e.fe_pass(beta, alpha, fam, lnk, init="multiple" if mode.get("mode") == 2 else "single")
    errs = dict(A=scaled_err(A, ref["A"]), b=nrel(b, ref["b"]), s=nrel(S, ref["S"]), t=nrel(t, ref["t"]),
                W=nrel(W, ref["W"]))
    if beta is not None and fam == "poisson" and lnk == "log":
        n = len(c["y"])
        mu = np.exp(c["X"] @ beta + kw["off"] + alpha[ids])
        dev = R.deviance("poisson", c["y"], mu, np.ones(n), kw["pw"], 1)
        errs["dev"] = abs(2.0 * s[L.S_DEV] - dev) / abs(dev)
        errs["sumw"] = abs(s[L.S_SUMW] - kw["pw"].sum()) / kw["pw"].sum()
    worst = max(errs.values())
    print(f"\nMARGIN {label}: {1e-9 / max(worst, 1e-300):.3g} (" + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) +
          f"; cond {downdate_cond(ref):.2e}, G {G})")
    assert np.array_equal(A, A.T)
    assert worst <= 1e-9, (label, errs)
    return ref


@pytest.mark.parametrize("p", SWEEP_P)
def test_fe_pass_at_a_non_converged_point(eng, p):
    """Every width of the segment sums and of the Gram pass over the group rows; rows that are no multiple of
    32 or of the tile; runs around 16, 64 and the tile, sorted and shuffled; many one-row segments at p = 65."""
    n = sweep_n(p)
    for pat in ("sorted", "shuffled") + (("interleaved", "two_level") if p == 65 else ()):
        c, ids, G, kw = case("poisson", "log", n, p, pat)
        load(eng, c, ids, G, kw)
        check_pass(f"fe_pass {n}x{p} {pat}", eng, c, ids, G, kw, "poisson", "log", c["beta"] * 0.8,
                   c["alpha"] * 0.5 + 0.1)
    check_pass(f"fe_pass init {n}x{p}", eng, c, ids, G, kw, "poisson", "log", None, None)


def check_fe_fit(label, e, c, ids, G, kw, fam, lnk, tol=1e-6, init="single", npart=1):
    p = c["X"].shape[1]
    o = FR.dummy_fit(c["X"], c["y"], ids, G, fam, lnk, tol=tol, npart=npart, **kw)
    assert LR.clearance(o.dev_trace, tol) >= 10.0, (label, np.abs(np.diff(o.dev_trace)))
    r = e.fit_glm_fe(fam, lnk, tol=tol, init=init, npart=npart)
    f = r.fit
    a0 = np.nan_to_num(o.coefs[p:])
    ref = FR.fe_pass(c["X"], c["y"], o.coefs[:p], a0, ids, G, fam, lnk, **kw)
    cond = downdate_cond(ref)
    want = dict(coefs=o.coefs[:p], stderr=o.stderr[:p], deviance=o.deviance, null_deviance=o.null_deviance,
                pearson=o.pearson, loglik=o.loglik, iter=o.iter)
    check_fit(label, f, want, cond)
    XD = FR.dummy_design(c["X"], ids, G)
    w = FR.rows(c["X"], c["y"], o.coefs[:p], a0, ids, fam, lnk, **kw)[0]
    dcond = float(np.linalg.cond(XD.T @ (w[:, None] * XD)))
    aerr = np.abs(r.alpha - o.coefs[p:]) / np.maximum(np.abs(o.coefs[p:]), 1e-300)
    abar = coef_bound(o.coefs[p:], dcond)
    terr = rel(f.dev_trace, o.dev_trace)
    print(f"MARGIN {label} alpha: {float(np.min(abar / np.maximum(aerr, 1e-300))):.3g} (dummy cond {dcond:.2e}); "
          f"trace: {1e-9 / max(terr, 1e-300):.3g}")
    assert np.all(aerr <= abar), (label, aerr.max())
    assert len(f.dev_trace) == o.iter + 1 and terr <= 1e-9, (label, terr)
    assert r.G_eff == G and r.df_residual == len(c["y"]) - p - G
    return r, o, cond


@pytest.mark.parametrize("p", SWEEP_P)
def test_poisson_fits_match_the_dummy_fit(eng, p):
    n = sweep_n(p)
    c, ids, G, kw = case("poisson", "log", n, p, "sorted")
    load(eng, c, ids, G, kw)
    check_fe_fit(f"poisson {n}x{p}", eng, c, ids, G, kw, "poisson", "log")


FAMILY_CASES = [("binomial", "logit", 1e-6), ("binomial", "probit", 1e-6), ("binomial", "cloglog", 1e-6),
                ("gamma", "log", 1e-7), ("gamma", "inverse", 1e-6), ("gaussian", "identity", 1e-6),
                ("poisson", "sqrt", 1e-7), ("negbin", "log", 1e-7)]


@pytest.mark.parametrize("fam,lnk,tol", FAMILY_CASES)
def test_every_family_matches_the_dummy_fit(eng, fam, lnk, tol):
    """3001 x 20, groups of 5-row runs: binomial with trials m, poisson / negbin with offset and prior; the
    linearly convergent non-canonical pairs at the tol their oracle trace is clear of."""
    c, ids, G, kw = case(fam, lnk, 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    check_fe_fit(f"{fam}/{lnk}", eng, c, ids, G, kw, fam, lnk, tol=tol)


def test_both_init_modes(eng):
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    one, _, _ = check_fe_fit("init single", eng, c, ids, G, kw, "poisson", "log")
    four, _, _ = check_fe_fit("init multiple", eng, c, ids, G, kw, "poisson", "log", init="multiple", npart=4)
    assert four.fit.npart == 4 and one.fit.npart == 1
    check_pass("fe_pass init multiple", eng, c, ids, G, kw, "poisson", "log", None, None, mode=2)


def test_vcov_fe_converged_and_perturbed(eng):
    """inv(A) and the covariance clustered on the factor against the beta block of the dummy design's, at the
    solution and at (beta + 0.05, alpha - 0.03) -- where the score sums no longer vanish within groups and the
    U_g xbar_g term of S_g carries most of the meat: leaving it out misses the reference by far more than the bar."""
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    load(eng, c, ids, G, kw)
    r = eng.fit_glm_fe("poisson", "log")
    n, p = c["X"].shape
    for label, beta, alpha in (("converged", r.fit.coefs, r.alpha), ("perturbed", r.fit.coefs + 0.05, r.alpha - 0.03)):
        ref = FR.fe_pass(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", **kw)
        cond = downdate_cond(ref)
        C0 = eng.vcov_fe(beta, alpha, "poisson", "log", cluster=False)
        _, Cd = FR.dummy_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", "HC0", False, **kw)
        e0 = scaled_err(C0, Cd)
        print(f"\nMARGIN vcov_fe {label} inv(A): {0.5 * v_bar(cond) / max(e0, 1e-300):.3g} (cond {cond:.2e})")
        assert e0 <= 0.5 * v_bar(cond) and np.array_equal(C0, C0.T)
        for t in ("HC0", "HC1"):
            for ca in (True, False):
                Vd, _ = FR.dummy_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", t, ca, **kw)
                V, M = eng.vcov_fe(beta, alpha, "poisson", "log", type=t, cadjust=ca, return_meat=True)
                e = scaled_err(V, Vd)
                print(f"MARGIN vcov_fe {label} {t} cadjust={ca}: {v_bar(cond) / max(e, 1e-300):.3g} (err {e:.2e})")
                assert e <= v_bar(cond) and np.array_equal(V, V.T), (label, t, ca, e)
        if label == "perturbed":
            wrong = FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", "HC0", False, correct=False, **kw)
            right = FR.fe_cov(c["X"], c["y"], beta, alpha, ids, G, "poisson", "log", "HC0", False, **kw)
            M = eng.vcov_fe(beta, alpha, "poisson", "log", type="HC0", cadjust=False, return_meat=True)[1]
            assert scaled_err(M, right["M"]) <= 1e-9
            assert scaled_err(wrong["M"], right["M"]) > 1e3 * 1e-9  # the uncorrected meat cannot pass
    # the standard errors of the fit are those of inv(A) at the solution's last solve: same bar
    assert rel(np.sqrt(np.diag(eng.vcov_fe(r.fit.coefs, r.alpha, "poisson", "log", cluster=False))), r.fit.stderr) < 1e-6


def test_combine_depth(eng):
    """One group of 80 001 one-row segments beside groups of 1 600 rows and a one-segment group: the scalar
    sums and the row sums go through one, two and three combine levels."""
    n, p = 160_001, 5
    i = np.arange(n)
    ids = np.where(i % 2 == 0, 0, 1 + (i // 2) % 50)
    ids[-1] = 51
    G = 52
    _, start, _ = L.cluster_plan(ids, G)
    assert len(start) - 1 == n
    c = FR.make_case("poisson", "log", n, p, ids, G, SEED)
    kw = dict(m=None, off=c["off"], pw=c["pw"])
    load(eng, c, ids, G, kw)
    check_pass("combine depth", eng, c, ids, G, kw, "poisson", "log", c["beta"] * 0.8, c["alpha"] * 0.5)


def test_a_group_of_zero_prior_weight(eng):
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    pw = kw["pw"].copy()
    dead = ids == 3
    pw[dead] = 0.0
    eng.set_data(c["X"], c["y"], offset=kw["off"], prior=pw)
    eng.set_clusters(ids, G)
    r = eng.fit_glm_fe("poisson", "log")
    assert np.isnan(r.alpha[3]) and np.sum(np.isnan(r.alpha)) == 1
    assert r.G_eff == G - 1 and r.df_residual == 3001 - 20 - (G - 1)
    keep = ~dead
    sub = np.where(ids[keep] > 3, ids[keep] - 1, ids[keep])
    eng.set_data(np.asfortranarray(c["X"][keep]), c["y"][keep], offset=kw["off"][keep], prior=pw[keep])
    eng.set_clusters(sub, G - 1)
    q = eng.fit_glm_fe("poisson", "log")
    assert q.fit.iter == r.fit.iter
    assert rel(r.fit.coefs, q.fit.coefs) < 1e-9 and rel(r.fit.stderr, q.fit.stderr) < 1e-9
    assert rel(np.delete(r.alpha, 3), q.alpha) < 1e-9 and rel(r.fit.deviance, q.fit.deviance) < 1e-9
    # the covariance reads the NaN as 0 and counts G_eff
    V = eng.vcov_fe(q.fit.coefs, q.alpha, "poisson", "log", type="HC1")
    eng.set_data(c["X"], c["y"], offset=kw["off"], prior=pw)
    eng.set_clusters(ids, G)
    V2 = eng.vcov_fe(r.fit.coefs, r.alpha, "poisson", "log", type="HC1")
    a_full = FR.adjustment(3001, 20, G, G - 1, "HC1", True)  # n and the cadjust's G differ, G_eff does not
    a_sub = FR.adjustment(len(sub), 20, G - 1, G - 1, "HC1", True)
    assert scaled_err(V2 * (a_sub / a_full), V) <= 1e-8


def test_uninformative_groups(eng, capsys):
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    y = c["y"].copy()
    y[(ids == 4) | (ids == 9)] = 0.0
    eng.set_data(c["X"], y, offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids, G)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match=r"2 group\(s\).*first is group 4"):
        eng.fit_glm_fe("poisson", "log")
    assert eng.stats()["passes"] == 0  # checked before the first pass
    names = [f"x{j}" for j in range(20)]
    xf = Frame({"one": np.ones(3001), **{nm: c["X"][:, j] for j, nm in enumerate(names)}})
    labels = np.array([f"g{k:02d}" for k in ids])
    obj = GLM.fit_fe(Frame({"y": y}), xf, Frame({"g": labels}), "poisson", "log", offset=Frame({"o": kw["off"]}),
                     prior=Frame({"w": kw["pw"]}))
    assert "2 fixed effect(s)" in capsys.readouterr().out
    assert obj.fe_dropped_groups == 2 and obj.fe_dropped_rows == int(np.sum((ids == 4) | (ids == 9)))
    assert obj.xnames == names and sorted(obj.fixef) == sorted(set(labels) - {"g04", "g09"})
    keep = (ids != 4) & (ids != 9)
    _, sub = np.unique(ids[keep], return_inverse=True)
    eng.set_data(np.asfortranarray(c["X"][keep]), y[keep], offset=kw["off"][keep], prior=kw["pw"][keep])
    eng.set_clusters(sub, G - 2)
    q = eng.fit_glm_fe("poisson", "log")
    assert np.array_equal(np.asarray(obj.coefs).reshape(-1), q.fit.coefs) and obj.dfResidual == q.df_residual
    assert np.array_equal(np.array([obj.fixef[k] for k in sorted(obj.fixef)]), q.alpha)
    # binomial: all y = m is uninformative too
    cb, idb, Gb, kwb = case("binomial", "logit", 3001, 20, "two_level")
    yb = cb["y"].copy()
    yb[idb == 6] = kwb["m"][idb == 6]
    eng.set_data(cb["X"], yb, m=kwb["m"])
    eng.set_clusters(idb, Gb)
    with pytest.raises(L.IllegalArgumentException, match=r"1 group\(s\).*y = m.*first is group 6"):
        eng.fit_glm_fe("binomial", "logit")


def test_structural_refusals(eng):
    lib = L.load()
    c, ids, G, kw = case("poisson", "log", 3001, 20, "two_level")
    X1 = np.asfortranarray(np.column_stack([np.ones(3001), c["X"]]))  # an intercept
    eng.set_data(X1, c["y"], offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids, G)
    with pytest.raises(L.MatrixSingularException, match="column 0"):
        eng.fit_glm_fe("poisson", "log")
    X2 = c["X"].copy(order="F")
    X2[:, 7] = np.random.default_rng(0).normal(size=G)[ids]  # constant within every group
    eng.set_data(X2, c["y"], offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids, G)
    with pytest.raises(L.MatrixSingularException, match="column 7"):
        eng.fit_glm_fe("poisson", "log")
    with pytest.raises(L.MatrixSingularException, match="column 7"):
        eng.vcov_fe(c["beta"], c["alpha"], "poisson", "log")
    load(eng, c, ids, G, kw)
    o = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0)
    cov = np.zeros((20, 20), order="F")
    for hc in (2, 3):
        assert lib.sglm_vcov_fe(eng._h, C.byref(o), L.ptr(c["beta"]), L.ptr(c["alpha"]), 1, hc, 1,
                                cov.ctypes.data_as(L.dp), None) == L.SGLM_EINVAL
    eng.set_clusters(None)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.fit_glm_fe("poisson", "log")
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.fe_pass(None, None, "poisson", "log")
    assert eng.stats()["passes"] == 0
    Xw, yw, _, _ = synth.generate(0, 0, 1000, 257, 3)
    eng.set_data(Xw, yw)
    eng.set_clusters(np.arange(1000) % 7, 7)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.fit_glm_fe("binomial", "logit")
    eng.synth(0, 0, 4096, 64, 5, procedural=True)
    eng.set_clusters(np.arange(4096) % 7, 7)
    with pytest.raises(L.IllegalArgumentException, match="procedural"):
        eng.fit_glm_fe("binomial", "logit")
    assert eng.stats()["passes"] == 0


N_BIG, P_BIG = 4001, 64


@pytest.fixture(scope="module")
def big(eng):
    out = {}
    for pat in ("interleaved", "sorted"):
        c, ids, G, kw = case("poisson", "log", N_BIG, P_BIG, pat, seed=4)  # (clear of tol for both patterns)
        load(eng, c, ids, G, kw)
        r, o, cond = check_fe_fit(f"big {pat}", eng, c, ids, G, kw, "poisson", "log")
        out[pat] = (c, ids, G, kw, r, cond)
    return out


def test_two_fits_are_bitwise_identical_and_nothing_else_moves(eng, big):
    c, ids, G, kw, one, cond = big["interleaved"]
    eng.set_data(c["X"], c["y"], offset=kw["off"], prior=kw["pw"])
    pick = lambda d: (d[0], d[1], d[3], d[4])  # X, y, offset, prior (no m was loaded)
    before = pick(eng.get_data())
    plain0 = eng.fit_glm("poisson", "log")
    eng.set_clusters(ids, G)
    plain1 = eng.fit_glm("poisson", "log")  # a handle that has clusters set fits as before
    a = eng.fit_glm_fe("poisson", "log")
    b = eng.fit_glm_fe("poisson", "log")
    for r in (a, b):
        assert np.array_equal(r.fit.coefs, one.fit.coefs) and np.array_equal(r.alpha, one.alpha)
        assert np.array_equal(r.fit.dev_trace, one.fit.dev_trace) and np.array_equal(r.fit.stderr, one.fit.stderr)
    ms = eng.fe_ms()
    assert len(ms) == 4 and all(v > 0.0 for v in ms)
    after = pick(eng.get_data())
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.array_equal(after[2], kw["off"])  # the user's offset
    plain2 = eng.fit_glm("poisson", "log")
    for f in (plain1, plain2):
        assert np.array_equal(f.coefs, plain0.coefs) and np.array_equal(f.stderr, plain0.stderr)
        assert np.array_equal(f.dev_trace, plain0.dev_trace) and f.iter == plain0.iter
    # the cluster-robust covariance shares the internal engine's design with the group rows: it still agrees
    V0 = eng.vcov_cluster(plain0.coefs, "poisson", "log")
    eng.fit_glm_fe("poisson", "log")
    assert np.array_equal(eng.vcov_cluster(plain0.coefs, "poisson", "log"), V0)


def assert_same_fit(label, r, one, cond):
    want = dict(coefs=one.fit.coefs, stderr=one.fit.stderr, deviance=one.fit.deviance,
                null_deviance=one.fit.null_deviance, pearson=one.fit.pearson, loglik=one.fit.loglik, iter=one.fit.iter)
    check_fit(label, r.fit, want, cond)
    assert rel(r.alpha, one.alpha) <= 1e-9 and r.G_eff == one.G_eff


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
@pytest.mark.parametrize("devices", ([0, 0], [0]))
def test_group_handle_matches_the_single_handle(big, devices, pat):
    """[0, 0]: two shards summed on the host; [0]: the RCCL group all-reduce.  Groups span the shard boundary
    (interleaved: every group; sorted: the one the boundary cuts).  Twice: the cross-shard sum of one step
    must not reach the next."""
    c, ids, G, kw, one, cond = big[pat]
    with Engine(devices=devices) as g:
        assert g.fe_ms() == (-1.0, -1.0, -1.0, -1.0)
        load(g, c, ids, G, kw)
        a = g.fit_glm_fe("poisson", "log")
        b = g.fit_glm_fe("poisson", "log")
        assert_same_fit(f"group {devices} {pat}", a, one, cond)
        assert np.array_equal(a.fit.coefs, b.fit.coefs) and np.array_equal(a.alpha, b.alpha)
        assert all(v > 0.0 for v in g.fe_ms())


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
def test_local_communicator_ranks_agree(eng, big, pat):
    c, ids, G, kw, one, cond = big[pat]
    load(eng, c, ids, G, kw)
    V1 = eng.vcov_fe(one.fit.coefs, one.alpha, "poisson", "log")
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(N_BIG, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(c["X"][lo:hi]), c["y"][lo:hi], offset=kw["off"][lo:hi],
                           prior=kw["pw"][lo:hi])
                e.set_clusters(ids[lo:hi], G)  # global codes
                fit = e.fit_glm_fe("poisson", "log")
                again = e.fit_glm_fe("poisson", "log")
                assert np.array_equal(fit.fit.coefs, again.fit.coefs) and np.array_equal(fit.alpha, again.alpha)
                res[r] = (fit, e.vcov_fe(fit.fit.coefs, fit.alpha, "poisson", "log"))
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    assert np.array_equal(res[0][0].fit.coefs, res[1][0].fit.coefs) and np.array_equal(res[0][0].alpha, res[1][0].alpha)
    assert np.array_equal(res[0][0].fit.dev_trace, res[1][0].fit.dev_trace) and np.array_equal(res[0][1], res[1][1])
    assert_same_fit(f"local comm {pat}", res[0][0], one, cond)
    assert scaled_err(res[0][1], V1) <= v_bar(cond)


def test_python_round_trip_on_iris(iris):
    """GLM.fit_fe with Species as the factor against GLM.fit with the three Species dummies."""
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    sp = iris["Species"]
    levels = sorted(set(sp))
    y = Frame({"Sepal_Width": iris["Sepal_Width"]})
    x = Frame({"(Intercept)": np.ones(len(sp)), "Petal_Length": iris["Petal_Length"], "Petal_Width": iris["Petal_Width"]})
    fe = Frame({"Species": sp})
    xd = Frame({"Petal_Length": iris["Petal_Length"], "Petal_Width": iris["Petal_Width"],
                **{f"Species_{l}": (sp == l).astype(float) for l in levels}})
    # (gamma / log converges linearly: its oracle trace is a factor 10 clear of 1e-8, not of the default tol)
    for fam, lnk, tol in (("gaussian", "identity", 1e-6), ("gamma", "log", 1e-8)):
        o = FR.dummy_fit(np.column_stack([iris["Petal_Length"], iris["Petal_Width"]]), iris["Sepal_Width"],
                         np.unique(sp, return_inverse=True)[1], 3, fam, lnk, tol=tol)
        assert LR.clearance(o.dev_trace, tol) >= 10.0
        obj = GLM.fit_fe(y, x, fe, fam, lnk, tol=tol)
        ref = GLM.fit(y, xd, fam, lnk, tol)
        rc = np.asarray(ref.coefs).reshape(-1)
        assert obj.xnames == ["Petal_Length", "Petal_Width"] and obj.iter == ref.iter
        assert rel(np.asarray(obj.coefs).reshape(-1), rc[:2]) < 1e-9 and rel(obj.stdErr, ref.stdErr[:2]) < 1e-9
        assert rel([obj.fixef[l] for l in levels], rc[2:]) < 1e-9
        assert rel([obj.deviance, obj.nullDeviance, obj.pearson, obj.loglik, obj.aic, obj.pDispersion],
                   [ref.deviance, ref.nullDeviance, ref.pearson, ref.loglik, ref.aic, ref.pDispersion]) < 1e-9
        assert obj.dfResidual == ref.dfResidual == 150 - 5 and obj.fe_dropped_groups == 0
        tab = GLM.coeftest(obj, y, x, fe=fe)
        want = GLM.coeftest(ref, y, xd, type="HC1", cluster=fe)
        assert list(tab["name"]) == obj.xnames
        assert rel(tab["se"], np.asarray(want["se"])[:2]) < 1e-8 and rel(tab["stat"], np.asarray(want["stat"])[:2]) < 1e-8
        assert rel(np.sqrt(np.diag(GLM.vcov_fe(obj, y, x, fe))), obj.stdErr) < 1e-9
        new = Frame({"Petal_Length": np.array([1.5, 4.0, 5.5]), "Petal_Width": np.array([0.2, 1.3, 2.0])})
        got = obj.predict(new, fe=Frame({"Species": np.array(["setosa", "versicolor", "unknown"], dtype=object)}))
        newd = Frame({"Petal_Length": new["Petal_Length"], "Petal_Width": new["Petal_Width"],
                      "Species_setosa": np.array([1.0, 0, 0]), "Species_versicolor": np.array([0, 1.0, 0]),
                      "Species_virginica": np.array([0, 0, 0.0])})
        want = ref.predict(newd)
        assert rel(got["value"][:2], want["value"][:2]) < 1e-9 and np.isnan(got["value"][2])
