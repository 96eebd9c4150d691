"""Two-way fixed-effects GLM fits on the GPU (sglm_set_fe2, sglm_fit_glm_fe2, sglm_fe2_pass, sglm_vcov_fe2: the
kernels of fe2.hip beside the one-way step's) against tests/fe2_reference.py: the dummy-variable IRLS on
[X | D1 | D2 without one column per component] and a numpy restatement of one concentrated step by another
route (rows demeaned by a dense lstsq on the dummy columns).

Bars (the one-way suite's):
  fe2_pass  A scaled_err <= 1e-9;  b, S1, S2, Y nrel <= 1e-9 (Y after its per-component null-space shift is
            removed);  scalars rel <= 1e-9;  A exactly symmetric
  fits      conftest.check_fit with cond = ||X'WX||_2 ||inv(A)||_2 (the downdate loses that factor); alpha and
            gamma against the dummy coefficients within coef_bound at the dummy Gram's cond; dev_trace elementwise
            1e-9; the iteration count where the oracle's trace is a factor 10 clear of tol; every margin >= 5
  V         scaled_err <= 2 max(1e-9, K_BOUND cond eps), inv(A) alone half of that

The reference's own error and the sweep tolerance's effect are asserted on the CPU (tests/test_fe2_reference.py):
at the default sweep_tol = 1e-12 the downdate is <= 1e-11 from the rows demeaned in np.longdouble.
"""
import ctypes as C

import numpy as np
import pytest

import fe2_reference as F2
import fe_reference as FR
import links_reference as LR
import np_reference as R
from conftest import K_BOUND, check_fit, coef_bound, nrel, rel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, _lib as L, synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
T = L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0]  # the engine's tile_rows (no device)
SWEEP_P = (1, 5, 16, 17, 33, 63, 64, 65, 129, 256)
SEED = 2


def v_bar(cond):
    return 2.0 * max(1e-9, K_BOUND * cond * EPS)


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def sweep_n(p):
    n = 2 * T + 1000 + 15 * (p % 7)
    assert n % T != 0
    return n


_cases = {}


def case(fam, lnk, n, p, pat2, pat1="sorted", seed=SEED, zero_weights=True):
    """The data of one case and its kwargs for the references, made once per module."""
    key = (fam, lnk, n, p, pat2, pat1, seed, zero_weights)
    if key not in _cases:
        ids1, G = FR.make_ids(pat1, n, T)
        ids2, H = F2.make_ids2(pat2, ids1, G)
        c = F2.make_case2(fam, lnk, n, p, ids1, G, ids2, H, seed, zero_weights=zero_weights)
        assert F2.drop_uninformative(ids1, ids2, c["y"], fam, c["m"], c["pw"])[0].all()
        kw = dict(m=c["m"], off=c["off"], pw=c["pw"])
        if fam == "negbin":
            kw["theta"] = 2.0
        _cases[key] = (c, ids1, G, ids2, H, kw)
    return _cases[key]


def load(e, c, ids1, G, ids2, H, kw):
    if "theta" in kw:
        e.set_theta(kw["theta"])
    e.set_data(c["X"], c["y"], m=kw["m"], offset=kw["off"], prior=kw["pw"])
    e.set_clusters(ids1, G)
    e.set_fe2(ids2, H)


def downdate_cond(ref):
    return float(np.linalg.norm(ref["XtWX"], 2) * np.linalg.norm(np.linalg.inv(ref["A"]), 2))


def check_pass(label, e, c, ids1, G, ids2, H, kw, fam, lnk, beta, alpha, gamma, mode=0):
    """fe2_pass at (beta, alpha, gamma) against the reference's A, b, level sums, Y and the pass's scalars."""
    mu0 = float(np.sum(c["y"])) / len(c["y"])
    ref = F2.fe2_pass(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, G, H, fam, lnk, mode=mode, mu0=mu0, **kw)
    r = e.fe2_pass(beta, alpha, gamma, fam, lnk, init="multiple" if mode == 2 else "single")
    p = c["X"].shape[1]
    Y0 = F2.remove_shift(F2.solve_K(ref["M"], ref["w"], ids1, ids2, G, H), ids1, ids2, G, H)
    errs = dict(A=scaled_err(r["A"], ref["A"]), b=nrel(r["b"], ref["b"]),
                S1=nrel(np.column_stack([r["S1"], r["t1"]]), ref["S1"]), W1=nrel(r["W1"], ref["W1"]),
                S2=nrel(np.column_stack([r["S2"], r["t2"]]), ref["S2"]), W2=nrel(r["W2"], ref["W2"]),
                Y=nrel(F2.remove_shift(r["Y"], ids1, ids2, G, H), Y0))
    if beta is not None and fam == "poisson" and lnk == "log":
        n = len(c["y"])
        mu = np.exp(c["X"] @ beta + kw["off"] + alpha[ids1] + gamma[ids2])
        dev = R.deviance("poisson", c["y"], mu, np.ones(n), kw["pw"], 1)
        errs["dev"] = abs(2.0 * r["scalars"][L.S_DEV] - dev) / abs(dev)
        errs["sumw"] = abs(r["scalars"][L.S_SUMW] - kw["pw"].sum()) / kw["pw"].sum()
    worst = max(errs.values())
    print(f"\nMARGIN {label}: {1e-9 / max(worst, 1e-300):.3g} (" + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) +
          f"; cond {downdate_cond(ref):.2e}, G {G}, H {H}, sweeps {r['sweeps']})")
    assert np.array_equal(r["A"], r["A"].T)
    assert worst <= 1e-9, (label, errs)
    return r


@pytest.mark.parametrize("p", SWEEP_P)
def test_fe2_pass_at_a_non_converged_point(eng, p):
    """Every width of the list sums, the gathers and the cross product (p + 1 and p + 2 columns cross the
    64-column slab at 63 / 64 / 65); rows that are no multiple of 32, of the tile or of the chunk; at p = 65 every
    factor-2 pattern and factor 1 shuffled as well (one-row segments)."""
    n = sweep_n(p)
    pats = [("cycle", "sorted"), ("random", "sorted")]
    if p == 65:
        pats += [(q, "sorted") for q in F2.PATTERNS2[2:]] + [("random", "shuffled"), ("cycle", "shuffled")]
    for pat2, pat1 in pats:
        c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, pat2, pat1, zero_weights=False)
        load(eng, c, ids1, G, ids2, H, kw)
        r = check_pass(f"fe2_pass {n}x{p} {pat1}/{pat2}", eng, c, ids1, G, ids2, H, kw, "poisson", "log",
                       c["beta"] * 0.8, c["alpha"] * 0.5 + 0.1, c["gamma"] * 0.5)
        if pat2 in ("nested", "single"):
            assert r["sweeps"] == 1
    check_pass(f"fe2_pass init {n}x{p}", eng, c, ids1, G, ids2, H, kw, "poisson", "log", None, None, None, mode=1)


def test_a_level_of_several_chunks_and_two_combine_levels(eng):
    """`giant` at 20 011 rows: the big level holds ~19 600 rows, 154 chunks, so its sums take a second combine
    level; the small levels are single chunks."""
    n, p = 20_011, 5
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "giant", zero_weights=False)
    plan = L.fe2_plan(ids1, ids2, G, H)
    assert np.sum(plan["chunk_level"] == 1) > 64
    load(eng, c, ids1, G, ids2, H, kw)
    check_pass("giant 20011x5", eng, c, ids1, G, ids2, H, kw, "poisson", "log", c["beta"] * 0.8, c["alpha"] * 0.5,
               c["gamma"] * 0.5)


def test_init_multiple_with_zero_weight_rows_and_a_partial_tile(eng):
    """The initial pass in mode "multiple" (beta = alpha = gamma = None) on binomial counts with m: t2 and W2 are
    sums over factor 2's lists of the per-row w z and w that the weights kernel stores -- several tiles, a last
    partial one, and rows of prior weight 0, which must store exact zeros."""
    n, p = sweep_n(5), 5
    c, ids1, G, ids2, H, kw = case("binomial", "logit", n, p, "random", "sorted", zero_weights=True)
    assert n > 2 * T and n % T != 0 and np.any(kw["pw"] == 0.0) and kw["m"] is not None
    load(eng, c, ids1, G, ids2, H, kw)
    check_pass(f"fe2_pass init multiple binomial {n}x{p}", eng, c, ids1, G, ids2, H, kw, "binomial", "logit",
               None, None, None, mode=2)


def test_uninformative_levels_of_factor_2_from_the_stored_row_values(eng):
    """The check's sums over factor 2 come from the y and 1 the weights kernel stores per row: one level with
    y = 0 on every row of positive weight, one whose only y > 0 sit on rows of prior weight 0; no level of
    factor 1 is uninformative, so the refusal is factor 2's, with numpy's count and first level."""
    n, p = sweep_n(5), 5
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random", "sorted", zero_weights=True)
    pw, y = kw["pw"], c["y"].copy()
    y[ids2 == 2] = 0.0
    y[(ids2 == 6) & (pw > 0.0)] = 0.0
    y[(ids2 == 6) & (pw == 0.0)] = 3.0
    assert np.any((ids2 == 6) & (pw == 0.0))

    def uninformative(ids, L):
        a, b = np.zeros(L), np.zeros(L)
        np.add.at(a, ids[pw > 0.0], y[pw > 0.0])
        np.add.at(b, ids[pw > 0.0], 1.0)
        return np.flatnonzero((a == 0.0) != (b == 0.0))

    assert len(uninformative(ids1, G)) == 0
    bad = uninformative(ids2, H)
    assert list(bad) == [2, 6]
    eng.set_data(c["X"], y, offset=kw["off"], prior=pw)
    eng.set_clusters(ids1, G)
    eng.set_fe2(ids2, H)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException,
                       match=rf"{len(bad)} level\(s\) of factor 2 have no finite fixed effect.*"
                             rf"first is level {bad[0]} of factor 2"):
        eng.fit_glm_fe2("poisson", "log")
    assert eng.stats()["passes"] == 0


def check_fe2_fit(label, e, c, ids1, G, ids2, H, kw, fam, lnk, tol=1e-6):
    p = c["X"].shape[1]
    n = len(c["y"])
    o, kept = F2.dummy_fit2(c["X"], c["y"], ids1, ids2, G, H, fam, lnk, tol=tol, **kw)
    b0, a0, g0 = F2.split_coefs(o.coefs, p, G, H, ids2, kept)
    clear = LR.clearance(o.dev_trace, tol) >= 10.0
    r = e.fit_glm_fe2(fam, lnk, tol=tol)
    f = r.fit
    refkw = {k: v for k, v in kw.items()}
    ref = F2.fe2_pass(c["X"], c["y"], b0, a0, g0, ids1, ids2, G, H, fam, lnk, **refkw)
    cond = downdate_cond(ref)
    want = dict(coefs=b0, stderr=o.stderr[:p], deviance=o.deviance, null_deviance=o.null_deviance,
                pearson=o.pearson, loglik=o.loglik)
    if np.isinf(o.loglik):
        # gaussian with rows of prior weight 0: the oracle's loglik is -inf (log of a zero weight), the engine's
        # statistics pass -- the one of fit_glm -- gives NaN there; neither is a number to compare
        assert fam == "gaussian" and not np.isfinite(f.loglik)
        del want["loglik"]
    if clear:
        want["iter"] = o.iter
    margin = check_fit(label, f, want, cond)
    XD, _ = F2.dummy_design2(c["X"], ids1, ids2, G, H)
    dcond = float(np.linalg.cond(XD.T @ (ref["w"][:, None] * XD)))
    eff, eff0 = np.concatenate([r.alpha, r.gamma[kept]]), np.concatenate([a0, g0[kept]])
    ebar = coef_bound(eff0, dcond)
    eerr = np.abs(eff - eff0) / np.maximum(np.abs(eff0), 1e-300)
    m_eff = float(np.min(ebar / np.maximum(eerr, 1e-300)))
    nit = min(len(f.dev_trace), len(o.dev_trace))
    terr = rel(f.dev_trace[:nit], o.dev_trace[:nit])
    m_trace = 1e-9 / max(terr, 1e-300)
    print(f"MARGIN {label} effects: {m_eff:.3g} (dummy cond {dcond:.2e}); trace: {m_trace:.3g}; sweeps {r.sweeps}; "
          f"clear of tol: {clear}")
    assert min(margin, m_eff, m_trace) >= 5.0, (label, margin, m_eff, m_trace)
    if clear:
        assert len(f.dev_trace) == o.iter + 1
    _, comp2, low = F2.components(ids1, ids2, G, H)
    assert np.all(r.gamma[low] == 0.0) and np.array_equal(np.isnan(r.gamma), comp2 < 0)
    return r, o, cond


@pytest.mark.parametrize("pat2", ("cycle", "random", "two_comp", "nested", "giant", "empty"))
def test_poisson_fits_match_the_dummy_fit(eng, pat2):
    """1346 x 20 with an offset and prior weights that include zeros; df_residual and ncomp where the level graph
    has more than one component or a code without rows."""
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, pat2)
    load(eng, c, ids1, G, ids2, H, kw)
    r, _, _ = check_fe2_fit(f"poisson {pat2}", eng, c, ids1, G, ids2, H, kw, "poisson", "log")
    ncomp = dict(cycle=1, random=1, two_comp=2, nested=4, giant=1, empty=1)[pat2]
    heff = H - 1 if pat2 == "empty" else H
    assert r.ncomp == ncomp and r.G_eff == G and r.H_eff == heff
    assert r.df_residual == n - p - (G + heff - ncomp)
    if pat2 == "nested":
        assert r.df_residual == n - p - G and r.sweeps[0] == 1


@pytest.mark.parametrize("fam,lnk,tol", [("binomial", "logit", 1e-6), ("gamma", "log", 1e-7),
                                         ("gaussian", "identity", 1e-6), ("negbin", "log", 1e-7)])
def test_every_family_matches_the_dummy_fit(eng, fam, lnk, tol):
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case(fam, lnk, n, p, "random")
    load(eng, c, ids1, G, ids2, H, kw)
    check_fe2_fit(f"{fam}/{lnk}", eng, c, ids1, G, ids2, H, kw, fam, lnk, tol=tol)


def test_single_level_second_factor_is_the_one_way_fit(eng):
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "single")
    load(eng, c, ids1, G, ids2, H, kw)
    one = eng.fit_glm_fe("poisson", "log")
    two = eng.fit_glm_fe2("poisson", "log")
    ref = F2.fe2_pass(c["X"], c["y"], one.fit.coefs, one.alpha, np.zeros(1), ids1, ids2, G, H, "poisson", "log", **kw)
    want = dict(coefs=one.fit.coefs, stderr=one.fit.stderr, deviance=one.fit.deviance,
                null_deviance=one.fit.null_deviance, pearson=one.fit.pearson, loglik=one.fit.loglik, iter=one.fit.iter)
    assert check_fit("single", two.fit, want, downdate_cond(ref)) >= 5.0
    assert two.sweeps[0] == 1 and two.sweeps[1] == two.fit.iter + 1
    assert rel(two.alpha, one.alpha) <= 1e-9 and two.gamma[0] == 0.0
    assert two.df_residual == one.df_residual and two.ncomp == 1


def test_vcov_fe2_converged_and_perturbed(eng):
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random")
    load(eng, c, ids1, G, ids2, H, kw)
    r = eng.fit_glm_fe2("poisson", "log")
    pa, pg = F2.normalise(r.alpha - 0.03, r.gamma + 0.02, ids1, ids2, G, H)
    for label, beta, alpha, gamma in (("converged", r.fit.coefs, r.alpha, r.gamma), ("perturbed", r.fit.coefs + 0.05, pa, pg)):
        ref = F2.fe2_pass(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, G, H, "poisson", "log", **kw)
        cond = downdate_cond(ref)
        C0 = eng.vcov_fe2(beta, alpha, gamma, "poisson", "log", cluster=False)
        _, Cd = F2.dummy_cov2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, G, H, "poisson", "log", "HC0", False, **kw)
        e0 = scaled_err(C0, Cd)
        print(f"\nMARGIN vcov_fe2 {label} inv(A): {0.5 * v_bar(cond) / max(e0, 1e-300):.3g} (cond {cond:.2e})")
        assert e0 <= 0.5 * v_bar(cond) and np.array_equal(C0, C0.T)
        for t in ("HC0", "HC1"):
            for ca in (True, False):
                Vd, _ = F2.dummy_cov2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, G, H, "poisson", "log", t, ca, **kw)
                V, M = eng.vcov_fe2(beta, alpha, gamma, "poisson", "log", type=t, cadjust=ca, return_meat=True)
                e = scaled_err(V, Vd)
                print(f"MARGIN vcov_fe2 {label} {t} cadjust={ca}: {v_bar(cond) / max(e, 1e-300):.3g} (err {e:.2e})")
                assert e <= v_bar(cond) and np.array_equal(V, V.T), (label, t, ca, e)
        _, _, u = F2.rows2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, "poisson", "log", **kw)
        assert scaled_err(M, F2.meat2(c["X"], u, ref["w"], ids1, ids2, G, H)) <= 1e-9
    assert rel(np.sqrt(np.diag(eng.vcov_fe2(r.fit.coefs, r.alpha, r.gamma, "poisson", "log", cluster=False))),
               r.fit.stderr) < 1e-6


def test_two_fits_are_bitwise_identical(eng):
    n, p = sweep_n(65), 65
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random")
    load(eng, c, ids1, G, ids2, H, kw)
    a = eng.fit_glm_fe2("poisson", "log")
    b = eng.fit_glm_fe2("poisson", "log")
    assert np.array_equal(a.fit.coefs, b.fit.coefs) and np.array_equal(a.fit.stderr, b.fit.stderr)
    assert np.array_equal(a.alpha, b.alpha) and np.array_equal(a.gamma, b.gamma, equal_nan=True)
    assert np.array_equal(a.fit.dev_trace, b.fit.dev_trace) and a.sweeps == b.sweeps and a.sweeps[0] > 1
    ms = eng.fe2_ms()
    assert len(ms) == 5 and all(v > 0.0 for v in ms)


def test_errors_before_any_launch(eng):
    lib = L.load()
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random")
    eng.set_data(c["X"], c["y"], offset=kw["off"], prior=kw["pw"])
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.set_fe2(ids2, H)  # the first factor comes first
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.fit_glm_fe2("poisson", "log")
    eng.set_clusters(ids1, G)
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_fe2"):
        eng.fit_glm_fe2("poisson", "log")
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_fe2"):
        eng.fe2_pass(None, None, None, "poisson", "log")
    with pytest.raises(L.IllegalArgumentException, match=r"\[0, H = 3\)"):
        eng.set_fe2(np.asarray(ids2, dtype=np.int32), 3)
    eng.set_fe2(ids2, H)
    eng.set_clusters(ids1, G)  # replacing the clusters drops the second factor
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_fe2"):
        eng.fit_glm_fe2("poisson", "log")
    eng.set_fe2(ids2, H)
    o = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0)
    fo = L.Fe2Opts(0.0, 0)
    cov = np.zeros((p, p), order="F")
    for hc in (2, 3):
        assert lib.sglm_vcov_fe2(eng._h, C.byref(o), C.byref(fo), L.ptr(c["beta"]), L.ptr(c["alpha"]), L.ptr(c["gamma"]),
                                 1, hc, 1, cov.ctypes.data_as(L.dp), None) == L.SGLM_EINVAL
        assert "HC2 / HC3" in L.last_error()
    assert eng.stats()["passes"] == 0
    # a wide design
    Xw, yw, _, _ = synth.generate(0, 0, 1000, 272, 3)
    eng.set_data(Xw, yw)
    eng.set_clusters(np.arange(1000) % 7, 7)
    eng.set_fe2(np.arange(1000) % 5, 5)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.fit_glm_fe2("binomial", "logit")
    assert eng.stats()["passes"] == 0
    # a multi-device handle, and a handle with a communicator
    with Engine(devices=[0, 0]) as g:
        g.set_data(c["X"], c["y"], offset=kw["off"], prior=kw["pw"])
        g.set_clusters(ids1, G)
        with pytest.raises(L.IllegalArgumentException, match="one device"):
            g.set_fe2(ids2, H)
        with pytest.raises(L.IllegalArgumentException, match="one device"):
            g.fit_glm_fe2("poisson", "log")
        assert g.stats()["passes"] == 0
    from sparkglm_amd import distributed as D
    comm = D.LocalComm(1)
    with Engine(0) as e1:
        e1.set_comm_local(comm.rank(0))
        e1.set_data(c["X"], c["y"], offset=kw["off"], prior=kw["pw"])
        e1.set_clusters(ids1, G)
        with pytest.raises(L.IllegalArgumentException, match="communicator"):
            e1.fit_glm_fe2("poisson", "log")
    comm.close()


def test_errors_of_the_step(eng):
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random")
    load(eng, c, ids1, G, ids2, H, kw)
    with pytest.raises(L.IllegalArgumentException, match=r"after 1 sweep\(s\) \(max_sweeps 1\)"):
        eng.fit_glm_fe2("poisson", "log", max_sweeps=1)
    X2 = c["X"].copy(order="F")
    X2[:, 7] = np.random.default_rng(0).normal(size=H)[ids2]  # constant within factor 2's levels
    eng.set_data(X2, c["y"], offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids1, G)
    eng.set_fe2(ids2, H)
    with pytest.raises(L.MatrixSingularException, match="column 7"):
        eng.fit_glm_fe2("poisson", "log")
    with pytest.raises(L.MatrixSingularException, match="column 7"):
        eng.vcov_fe2(c["beta"], c["alpha"], c["gamma"], "poisson", "log")
    y = c["y"].copy()
    y[ids2 == 4] = 0.0
    eng.set_data(c["X"], y, offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids1, G)
    eng.set_fe2(ids2, H)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match=r"1 level\(s\) of factor 2.*first is level 4 of factor 2"):
        eng.fit_glm_fe2("poisson", "log")
    assert eng.stats()["passes"] == 0  # checked before the first pass
    y = c["y"].copy()
    y[ids1 == 3] = 0.0
    eng.set_data(c["X"], y, offset=kw["off"], prior=kw["pw"])
    eng.set_clusters(ids1, G)
    eng.set_fe2(ids2, H)
    with pytest.raises(L.IllegalArgumentException, match=r"1 level\(s\) of factor 1.*first is level 3 of factor 1"):
        eng.fit_glm_fe2("poisson", "log")


def test_nothing_else_moves(eng):
    """After a two-way fit, fit_glm, fit_glm_fe and vcov_cluster on the same handle give bitwise their results from
    before it, and the resident data are untouched."""
    n, p = sweep_n(20), 20
    c, ids1, G, ids2, H, kw = case("poisson", "log", n, p, "random")
    load(eng, c, ids1, G, ids2, H, kw)
    pick = lambda d: (d[0], d[1], d[3], d[4])
    before = pick(eng.get_data())
    plain0 = eng.fit_glm("poisson", "log")
    one0 = eng.fit_glm_fe("poisson", "log")
    V0 = eng.vcov_cluster(plain0.coefs, "poisson", "log")
    two = eng.fit_glm_fe2("poisson", "log")
    eng.vcov_fe2(two.fit.coefs, two.alpha, two.gamma, "poisson", "log")
    plain1 = eng.fit_glm("poisson", "log")
    one1 = eng.fit_glm_fe("poisson", "log")
    assert np.array_equal(plain1.coefs, plain0.coefs) and np.array_equal(plain1.stderr, plain0.stderr)
    assert np.array_equal(plain1.dev_trace, plain0.dev_trace)
    assert np.array_equal(one1.fit.coefs, one0.fit.coefs) and np.array_equal(one1.alpha, one0.alpha)
    assert np.array_equal(one1.fit.dev_trace, one0.fit.dev_trace) and np.array_equal(one1.fit.stderr, one0.fit.stderr)
    assert np.array_equal(eng.vcov_cluster(plain0.coefs, "poisson", "log"), V0)
    for x, y in zip(before, pick(eng.get_data())):
        assert np.array_equal(x, y)


def test_python_round_trip_on_iris(iris, capsys):
    """GLM.fit_fe(fe2=) with Species and a four-level period against GLM.fit with their dummies; then a poisson
    fit where dropping a period's all-zero rows is reported."""
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    sp = iris["Species"]
    n = len(sp)
    per = np.array([f"q{k}" for k in (np.arange(n) * 7) % 4])
    levels, periods = sorted(set(sp)), sorted(set(per))
    y = Frame({"Sepal_Width": iris["Sepal_Width"]})
    x = Frame({"(Intercept)": np.ones(n), "Petal_Length": iris["Petal_Length"], "Petal_Width": iris["Petal_Width"]})
    fe, fe2 = Frame({"Species": sp}), Frame({"period": per})
    xd = Frame({"Petal_Length": iris["Petal_Length"], "Petal_Width": iris["Petal_Width"],
                **{f"Species_{l}": (sp == l).astype(float) for l in levels},
                **{f"period_{q}": (per == q).astype(float) for q in periods[1:]}})
    obj = GLM.fit_fe(y, x, fe, "gaussian", "identity", fe2=fe2)
    ref = GLM.fit(y, xd, "gaussian", "identity", 1e-6)
    rc = np.asarray(ref.coefs).reshape(-1)
    assert obj.xnames == ["Petal_Length", "Petal_Width"] and obj.iter == ref.iter
    assert rel(np.asarray(obj.coefs).reshape(-1), rc[:2]) < 1e-9 and rel(obj.stdErr, ref.stdErr[:2]) < 1e-9
    assert rel([obj.fixef[l] for l in levels], rc[2:5]) < 1e-9
    assert obj.fixef2[periods[0]] == 0.0 and rel([obj.fixef2[q] for q in periods[1:]], rc[5:]) < 1e-8
    assert rel([obj.deviance, obj.nullDeviance, obj.pearson, obj.loglik, obj.aic, obj.pDispersion],
               [ref.deviance, ref.nullDeviance, ref.pearson, ref.loglik, ref.aic, ref.pDispersion]) < 1e-9
    assert obj.dfResidual == ref.dfResidual == n - 2 - (3 + 4 - 1) and obj.fe_ncomp == 1 and obj.fe_dropped_groups == 0
    tab = GLM.coeftest(obj, y, x, fe=fe, fe2=fe2)
    want = GLM.coeftest(ref, y, xd, type="HC1", cluster=fe)
    assert rel(tab["se"], np.asarray(want["se"])[:2]) < 1e-8
    assert rel(np.sqrt(np.diag(GLM.vcov_fe(obj, y, x, fe, fe2=fe2))), obj.stdErr) < 1e-9
    new = Frame({"Petal_Length": np.array([1.5, 4.0, 5.5]), "Petal_Width": np.array([0.2, 1.3, 2.0])})
    got = obj.predict(new, fe=Frame({"Species": np.array(["setosa", "versicolor", "virginica"], dtype=object)}),
                      fe2=Frame({"period": np.array(["q1", "q0", "nope"], dtype=object)}))
    lin = lambda i, s, q: new["Petal_Length"][i] * rc[0] + new["Petal_Width"][i] * rc[1] + rc[2 + s] + q
    assert rel(got["value"][:2], [lin(0, 0, rc[5]), lin(1, 1, 0.0)]) < 1e-8 and np.isnan(got["value"][2])
    # poisson counts with one period all zero: its rows go, with a note
    cnt = np.round(iris["Sepal_Width"] * 2.0)
    cnt[per == "q2"] = 0.0
    capsys.readouterr()
    pois = GLM.fit_fe(Frame({"c": cnt}), x, fe, "poisson", "log", fe2=fe2)
    assert f"1 fixed effect(s) ({int(np.sum(per == 'q2'))} rows)" in capsys.readouterr().out
    assert sorted(pois.fixef2) == ["q0", "q1", "q3"] and pois.fe_dropped_rows == int(np.sum(per == "q2"))
