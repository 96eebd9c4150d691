"""The negative binomial family on every GPU pass path and MASS::glm.nb's theta estimation, against the numpy /
scipy reference tests/negbin_reference.py (pinned to the likelihood by tests/test_negbin_reference.py).

Shapes: tests/test_gpu_links.py's -- narrow P16 = 1..4, K1 at 5 and 6 column blocks, K1r at 10 and 13 and at the
odd count 5 (SGLM_FUSED_SPLIT=5), the wide path resident and procedural; n is never a multiple of a row block.
negbin / log (the pair with an inline row stage) runs at all of them, sqrt and identity (the run-time-link rows)
at one narrow, one K1, one K1r and the wide shape; theta varies over the cases (0.5, 3, 50 among them).

Every case first asserts, of the reference alone, that no row leaves the range at any iteration and that every
stopping decision is clear of its threshold (links_reference.trajectory_ok and its factor-10 / 1.5 rule); counts
of iterations are then compared exactly."""
import functools
import threading

import numpy as np
import pytest

import links_reference as LR
import negbin_reference as NB
from conftest import K_BOUND, check_fit, gram_cond, rel
from sandwich_reference import h_amp, scaled_err
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D
from test_gpu_influence import check_hat, check_resid
from test_gpu_links import _engine, _same

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
THETAS = (0.5, 3.0, 50.0, 1.7, 8.0)
# (n, p, SGLM_FUSED_SPLIT or None, kernel kind, links)
ALL = ("log", "sqrt", "identity")
SHAPES = [
    (3001, 16, None, "narrow", ("log",)),
    (3001, 20, None, "narrow", ALL),
    (4001, 33, None, "narrow", ("log",)),
    (6001, 64, None, "narrow", ("log",)),
    (6001, 70, None, "fused", ALL),
    (6001, 96, None, "fused", ("log",)),
    (6001, 150, None, "fused-split", ALL),
    (6001, 200, None, "fused-split", ("log",)),
    (6001, 70, 5, "fused-split", ("log",)),
    (5001, 290, None, "wide", ALL),
]
# theta cycles over THETAS.  One exception, decided on the reference alone: sqrt at 5001 x 290 with theta = 0.5
# (17 rows per column of counts that overdispersed) has no valid fit -- the reference itself leaves the range
# at every seed tried -- so that case takes theta = 8; sqrt meets theta = 0.5 at 6001 x 70.
THETA_OF = {("sqrt", 5001, 290): 8.0}
CASES = [(n, p, fs, kind, lnk, THETA_OF.get((lnk, n, p), THETAS[(i + ALL.index(lnk)) % len(THETAS)]))
         for i, (n, p, fs, kind, links) in enumerate(SHAPES) for lnk in links]
IDS = [f"{lnk}-theta{th:g}-{n}x{p}{'-split' + str(fs) if fs else ''}" for n, p, fs, kind, lnk, th in CASES]


def test_the_cases_cover_the_thetas():
    assert {0.5, 3.0, 50.0} <= {c[5] for c in CASES if c[4] == "log"}
    assert len(CASES) == 18


@functools.lru_cache(maxsize=None)
def _ref(lnk, n, p, theta):
    """The inputs of a fixed-theta case and the reference's fits (single and multiple init), computed once."""
    # (seeds chosen on the reference alone: identity at 6001 x 150 converges linearly at a rate that leaves no tol
    # of the list clear of its steps under the default seed)
    seed = {("identity", 6001, 150): 650}.get((lnk, n, p), 100 + p)
    X, y, off, pr, _ = NB.make_case(lnk, n, p, theta, seed)
    kw = dict(offset=off, prior=pr)
    traces = [NB.fit_glm(X, y, theta, lnk, tol=1e-11, max_iter=40, npart=g, **kw).dev_trace for g in (1, 2)]
    tol, clear = LR.pick_tol(traces)
    fits = {"single": NB.fit_glm(X, y, theta, lnk, tol=tol, npart=1, max_iter=60, **kw),
            "multiple": NB.fit_glm(X, y, theta, lnk, tol=tol, npart=2, max_iter=60, **kw)}
    return dict(X=X, y=y, off=off, pr=pr, tol=tol, traces=traces, fits=fits, clear=clear, theta=theta)


def _assert_inputs(c, label):
    """Conditions on the test's inputs (the reference alone), not measurements."""
    for f in c["fits"].values():
        assert max(f.invalid) == 0, (label, f.invalid)
    print(f"\nINPUT {label}: tol {c['tol']:g}, clearance {c['clear']:.1f}, iterations "
          f"{c['fits']['single'].iter} / {c['fits']['multiple'].iter}")
    assert LR.trajectory_ok(c["traces"], c["tol"]), (label, c["tol"], c["clear"])


# ---- 1. fixed theta on every pass path ----
@pytest.mark.parametrize("n,p,fs,kind,lnk,theta", CASES, ids=IDS)
def test_fixed_theta_fit_on_every_pass_path(n, p, fs, kind, lnk, theta):
    label = f"negbin({theta:g})/{lnk} {n}x{p}" + (f" split{fs}" if fs else "")
    c = _ref(lnk, n, p, theta)
    _assert_inputs(c, label)
    want_kind, want_name = L.pass_kernel_for(n, p, "negbin", lnk, fused_split=fs or 1)
    assert want_kind == kind
    assert ("negbin,log>" if lnk == "log" else "negbin,runtime>") in want_name or kind == "wide"
    fits = {}
    for spec in (1, 0):
        with _engine({"SGLM_FUSED_SPLIT": fs, "SGLM_SPECULATE": spec}) as e:
            e.set_data(c["X"], c["y"], offset=c["off"], prior=c["pr"])
            if spec:
                with pytest.raises(L.IllegalArgumentException, match="theta"):  # no theta on the handle yet
                    e.fit_glm("negbin", lnk)
                assert e.get_theta() == 0.0
            e.set_theta(theta)
            assert e.get_theta() == theta
            for init in ("single", "multiple"):
                e.reset_stats()
                f = fits[spec, init] = e.fit_glm("negbin", lnk, tol=c["tol"], init=init)
                st = e.stats()
                if spec:
                    assert st["pass_kernel_name"] == want_name and st["pass_kernel_kind"] == kind
                    print(f"PASSES {label} {init}: {st['passes']} passes, {st['dev_passes']} deviance-only, "
                          f"{f.iter} iterations")
                    check_fit(f"{label} {init}", f, c["fits"][init], gram_cond(e, f.coefs, "negbin", lnk), tol=1e-9)
            if spec:  # one pass twice: bitwise
                a = e.irls_pass(f.coefs, family="negbin", link=lnk)
                b = e.irls_pass(f.coefs, family="negbin", link=lnk)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
                assert np.isfinite(a[2][L.S_DEV]) and a[2][L.S_BAD] == 0
    for init in ("single", "multiple"):  # the speculative last pass is bitwise neutral
        _same(fits[1, init], fits[0, init])


def test_procedural_wide_fit():
    """negbin / log on the count design of synth kind 2, generated in the kernels, against the reference on the
    host-generated design."""
    n, p, theta = 6000, 520, 3.0
    X, y, off, pr = synth.generate(2, 0, n, p, 11)
    kw = dict(offset=off, prior=pr)
    traces = [NB.fit_glm(X, y, theta, "log", tol=1e-11, max_iter=40, npart=g, **kw).dev_trace for g in (1, 2)]
    tol, clear = LR.pick_tol(traces)
    c = dict(tol=tol, clear=clear, traces=traces,
             fits={i: NB.fit_glm(X, y, theta, "log", tol=tol, npart=g, max_iter=60, **kw)
                   for i, g in (("single", 1), ("multiple", 2))})
    _assert_inputs(c, "procedural negbin/log")
    with Engine(0) as e:
        e.synth(2, 0, n, p, 11, procedural=True)
        e.set_theta(theta)
        for init in ("single", "multiple"):
            f = e.fit_glm("negbin", "log", tol=tol, init=init)
            assert e.stats()["pass_kernel_kind"] == "wide-procedural"
            check_fit(f"procedural negbin/log {init}", f, c["fits"][init], gram_cond(e, f.coefs, "negbin", "log"))


# ---- 2. the theta terms ----
def _terms_case(n, lnk="log"):
    """Rows with mu in about [1, 6], overdispersed counts, the hand-placed counts 0, 1, 2, 170, 100000 and some
    zero prior weights (one of them on a hand-placed row)."""
    rng = np.random.default_rng(1000 + n)
    p = 3
    X = np.asfortranarray(np.column_stack([np.ones(n), rng.uniform(-1, 1, (n, p - 1))]))
    beta = np.array([{"log": 1.0, "sqrt": 1.7, "identity": 3.0}[lnk], 0.4, -0.3])
    off = rng.uniform(-0.05, 0.05, n)
    mu = LR.unlink("negbin", lnk, X @ beta + off, 1.0)
    y = rng.poisson(mu * rng.gamma(2.0, 0.5, n)).astype(np.float64)
    pw = 0.5 + rng.uniform(size=n)
    special = [0.0, 1.0, 2.0, 170.0, 100000.0]
    for k, v in enumerate(special[: n]):
        y[(k * 7) % n] = v
    if n > 8:
        pw[::5] = 0.0
        pw[(3 * 7) % n] = 1.25          # the row holding 170 keeps a weight
        pw[(4 * 7) % n] = 0.0 if n == 65 else pw[(4 * 7) % n]   # ... and at one size the 100000 row has none
    return X, y, off, pw, beta, mu


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3001, 70001])
def test_theta_terms_against_scipy(n):
    """The sums over n rows against the same formula in scipy double, at 1e-9 of `norm` (the operand magnitudes of
    the ungrouped score).  That reference cancels as the formula does, so this bar cannot be tighter: at
    theta = 1e4 it is twice the whole score.  What the rows are good to, per row and at a large theta, is held by
    tests/test_gpu_theta_rows.py against exact values."""
    X, y, off, pw, beta, mu = _terms_case(n)
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        worst = np.inf
        for theta in (0.01, 0.7, 30.0, 1e4):
            got = e.theta_terms(beta, theta, "log")
            assert np.array_equal(got, e.theta_terms(beta, theta, "log"))  # run to run: bitwise
            score, info, ll, mom, sw, norm = NB.theta_terms(y, mu, pw, theta)
            errs = dict(score=abs(got[0] - score) / norm, info=abs(got[1] - info) / abs(info),
                        loglik=abs(got[2] - ll) / abs(ll), mom=abs(got[3] - mom) / abs(mom), sumw=abs(got[4] - sw) / sw)
            margin = min(1e-9 / max(v, 1e-300) for v in errs.values())
            worst = min(worst, margin)
            print(f"\nMARGIN theta terms n={n} theta={theta:g}: {margin:.3g} "
                  + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
            assert margin >= 1.0, (n, theta, errs)


@pytest.mark.parametrize("lnk", ["sqrt", "identity"])
def test_theta_terms_other_links(lnk):
    X, y, off, pw, beta, mu = _terms_case(3001, lnk)
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        for theta in (0.7, 30.0):
            got = e.theta_terms(beta, theta, lnk)
            score, info, ll, mom, sw, norm = NB.theta_terms(y, mu, pw, theta)
            errs = [abs(got[0] - score) / norm, abs(got[1] - info) / abs(info), abs(got[2] - ll) / abs(ll)]
            print(f"\nMARGIN theta terms {lnk} theta={theta:g}: {1e-9 / max(max(errs), 1e-300):.3g}")
            assert max(errs) <= 1e-9, (lnk, theta, errs)


# ---- 3. theta.ml ----
@pytest.mark.parametrize("lnk,theta_star", [("log", 2.0), ("log", 0.6), ("sqrt", 3.0)])
def test_theta_ml(lnk, theta_star):
    n, p = 6001, 20
    X, y, off, pw, _ = NB.make_case(lnk, n, p, theta_star, 31)
    beta = LR.fit_glm(X, y, "poisson", lnk, offset=off, prior=pw, tol=1e-8).coefs
    mu = LR.unlink("negbin", lnk, X @ beta + off, 1.0)
    runs = {eps: NB.theta_ml(y, mu, pw, 25, eps) for eps in NB.THETA_EPSS}
    eps = next((e_ for e_ in NB.THETA_EPSS if NB.theta_clearance(runs[e_], e_) >= LR.CLEAR_FULL), None)
    if eps is None:
        eps = max(NB.THETA_EPSS, key=lambda e_: NB.theta_clearance(runs[e_], e_))
    o = runs[eps]
    clear = NB.theta_clearance(o, eps)
    print(f"\nINPUT theta.ml {lnk}: eps 2^{int(np.log2(eps))}, clearance {clear:.1f}, {o.iters} iterations, "
          f"theta {o.theta:.6f}")
    assert o.warn == 0 and clear >= LR.CLEAR_MIN
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        r = e.theta_ml(beta, lnk, limit=25, eps=eps)
        assert e.get_theta() == 0.0  # the handle's theta is not touched
    errs = (abs(r.theta - o.theta) / o.theta, abs(r.se - o.se) / o.se)
    print(f"MARGIN theta.ml {lnk}: {1e-9 / max(max(errs), 1e-300):.3g} (theta {errs[0]:.1e}, se {errs[1]:.1e})")
    assert (r.iters, r.warn) == (o.iters, o.warn)
    assert max(errs) <= 1e-9


def test_theta_ml_reports_the_iteration_limit():
    """Underdispersed counts (synth kind 2: floor(u 2 lambda)): the score stays positive and theta grows without
    bound, so the reference itself ends at limit = 3."""
    X, y, off, pw = synth.generate(2, 0, 5001, 20, 11)
    beta = LR.fit_glm(X, y, "poisson", "log", offset=off, prior=pw, tol=1e-8).coefs
    mu = np.exp(X @ beta + off)
    o = NB.theta_ml(y, mu, pw, 3, NB.THETA_EPS)
    assert o.warn == 1 and o.iters == 3
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        r = e.theta_ml(beta, "log", limit=3)
    assert (r.iters, r.warn) == (3, 1)
    assert abs(r.theta - o.theta) <= 1e-9 * o.theta


# ---- 4. the warm-started fit ----
@pytest.mark.parametrize("fam", ["poisson", "negbin"])
def test_fit_glm_start(fam):
    n, p, theta = 6001, 70, 3.0
    c = _ref("log", n, p, theta)
    X, y, off, pw = c["X"], c["y"], c["off"], c["pr"]
    kw = dict(offset=off, prior=pw)
    if fam == "negbin":
        ref = lambda start, tol, **k: NB.fit_glm(X, y, theta, "log", start=start, tol=tol, **kw, **k)
        cold = NB.fit_glm(X, y, theta, "log", tol=1e-11, max_iter=40, **kw)
    else:
        ref = lambda start, tol, **k: NB.fit_start(X, y, "poisson", "log", start, tol=tol, **kw, **k)
        cold = LR.fit_glm(X, y, "poisson", "log", tol=1e-11, max_iter=40, **kw)
    rng = np.random.default_rng(9)
    starts = {"converged": cold.coefs, "perturbed": cold.coefs + 0.05 * rng.uniform(-1, 1, p) * np.abs(cold.coefs).max()}
    with Engine(0) as e:
        e.set_data(X, y, **kw)
        e.set_theta(theta)
        cond = gram_cond(e, cold.coefs, fam, "log")
        for name, start in starts.items():
            long = ref(start, 1e-11, max_iter=40).dev_trace
            tol, clear = LR.pick_tol([long])
            o = ref(start, tol)
            print(f"\nINPUT start {fam} {name}: tol {tol:g}, clearance {clear:.1f}, {o.iter} iterations")
            assert LR.trajectory_ok([long], tol)
            if name == "converged":
                assert o.iter in (1, 2)
            f = e.fit_glm(fam, "log", tol=tol, start=start)
            check_fit(f"start {fam} {name}", f, o, cond)
            assert len(f.dev_trace) == len(o.dev_trace)
            assert rel(f.dev_trace, o.dev_trace) <= 1e-9
        with pytest.raises(L.IllegalArgumentException, match="Dimension mismatch"):
            e.fit_glm(fam, "log", start=np.zeros(p + 1))


# ---- 5. glm.nb ----
NB_CASES = [(6001, 20, "log", 2.0), (6001, 70, "log", 0.8), (6001, 150, "log", 5.0), (5001, 290, "log", 2.0),
            (6001, 20, "sqrt", 3.0)]


@functools.lru_cache(maxsize=None)
def _nb_ref(n, p, lnk, theta_star, npart=1):
    """A glm.nb case whose every stopping decision -- each inner |delta deviance| against tol, each Newton |del|
    against theta_eps, each outer quantity against epsilon -- is clear of its threshold; the three thresholds
    are picked from their short lists as links_reference.pick_tol picks tol."""
    X, y, off, pw, _ = NB.make_case(lnk, n, p, theta_star, 200 + p)
    kw = dict(offset=off, prior=pw, npart=npart)

    def worst(r, tol, teps, eps):
        inner = min(LR.clearance(t, tol) for t in r.inner_traces)
        newton = min(NB.theta_clearance(t, teps) for t in r.theta_runs)
        outer = NB.threshold_clearance(r.outer_stop, eps)
        return min(inner, newton, outer), (inner, newton, outer)

    # One threshold at a time, each from its list in order (the first that is a factor 10 clear, else the
    # clearest), the other two held; the sweep is repeated until it changes nothing, so that every choice -- and
    # whether any value of its list reaches the factor 10 -- is judged with the other two at their final values.
    pick = [LR.TOLS[0], NB.THETA_EPSS[0], NB.EPSILONS[0]]
    runs = {}

    def run():
        key = tuple(pick)
        if key not in runs:
            runs[key] = NB.glm_nb(X, y, lnk, tol=pick[0], theta_eps=pick[1], epsilon=pick[2], inner_max_iter=60, **kw)
        return runs[key]

    settled, none_full = False, [False, False, False]
    for sweep in range(4):
        before = list(pick)
        for k, cands in enumerate((LR.TOLS, NB.THETA_EPSS, NB.EPSILONS)):
            clear = {}
            none_full[k] = False
            for v in cands:
                pick[k] = v
                r = run()
                ok = r.converged and not any(t.warn for t in r.theta_runs)
                clear[v] = worst(r, *pick)[1][k] if ok else 0.0
                if clear[v] >= LR.CLEAR_FULL:
                    break
            else:
                pick[k] = max(clear, key=clear.get)
                none_full[k] = True
        if pick == before:
            settled = True
            break
    r = run()
    w, parts = worst(r, *pick)
    return dict(X=X, y=y, off=off, pw=pw, tol=pick[0], teps=pick[1], eps=pick[2], ref=r, clear=w, parts=parts,
                settled=settled, none_full=tuple(none_full))


def _assert_nb_inputs(c, label):
    r = c["ref"]
    print(f"\nINPUT {label}: tol {c['tol']:g}, theta_eps 2^{int(np.log2(c['teps']))}, epsilon {c['eps']:g}; clearance "
          f"{c['clear']:.1f} (inner {c['parts'][0]:.1f}, newton {c['parts'][1]:.1f}, outer {c['parts'][2]:.1f}); outer "
          f"{r.outer_iter}, last inner {r.fit.iter}, theta {r.theta:.6f}")
    assert r.converged and all(t.warn == 0 for t in r.theta_runs)
    assert all(max(getattr(f, "invalid", [0]) or [0]) == 0 for f in (r.fit0, r.fit))
    # links_reference's rule (trajectory_ok), per threshold with the other two at their final values: a factor 10,
    # or -- only where no value of that threshold's list reaches it -- at least 1.5
    assert c["settled"], label
    for name, part, none in zip(("inner", "newton", "outer"), c["parts"], c["none_full"]):
        assert part >= LR.CLEAR_FULL or (none and part >= LR.CLEAR_MIN), (label, name, part, none)


def _check_nb(label, r, e, c, cond):
    o = c["ref"]
    check_fit(label, r.fit, o.fit, cond)
    errs = dict(theta=abs(r.theta - o.theta) / o.theta, se=abs(r.se_theta - o.se_theta) / o.se_theta,
                twologlik=abs(r.twologlik - o.twologlik) / abs(o.twologlik))
    print(f"MARGIN {label} theta: {1e-9 / max(max(errs.values()), 1e-300):.3g} "
          + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-9, (label, errs)
    assert (r.outer_iter, r.fit.iter, r.converged, r.theta_warn) == (o.outer_iter, o.fit.iter, True, 0)
    assert e.get_theta() == r.theta


@pytest.mark.parametrize("n,p,lnk,theta_star", NB_CASES, ids=[f"{l}-{n}x{p}" for n, p, l, t in NB_CASES])
def test_fit_glm_nb(n, p, lnk, theta_star):
    label = f"glm.nb {lnk} {n}x{p}"
    c = _nb_ref(n, p, lnk, theta_star)
    _assert_nb_inputs(c, label)
    with Engine(0) as e:
        e.set_data(c["X"], c["y"], offset=c["off"], prior=c["pw"])
        r = e.fit_glm_nb(lnk, tol=c["tol"], epsilon=c["eps"], theta_eps=c["teps"])
        cond = gram_cond(e, r.fit.coefs, "negbin", lnk)
        _check_nb(label, r, e, c, cond)
        again = e.fit_glm_nb(lnk, tol=c["tol"], epsilon=c["eps"], theta_eps=c["teps"])
        assert again.theta == r.theta and np.array_equal(again.fit.coefs, r.fit.coefs)


def test_glm_nb_on_a_group_handle_and_two_local_ranks():
    n, p, lnk = 6001, 70, "log"
    c = _nb_ref(n, p, lnk, 0.8, npart=2)
    _assert_nb_inputs(c, "glm.nb multi")
    X, y, off, pw = c["X"], c["y"], c["off"], c["pw"]
    kw = dict(tol=c["tol"], epsilon=c["eps"], theta_eps=c["teps"], init="multiple")
    with Engine(0) as one:
        one.set_data(X, y, offset=off, prior=pw)
        r1 = one.fit_glm_nb(lnk, **kw)
        cond = gram_cond(one, r1.fit.coefs, "negbin", lnk)
        _check_nb("glm.nb one device", r1, one, c, cond)
    with Engine(devices=[0, 0]) as g:
        g.set_data(X, y, offset=off, prior=pw)
        rg = g.fit_glm_nb(lnk, **kw)
        _check_nb("glm.nb group[0, 0]", rg, g, c, cond)
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(n, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi], offset=off[lo:hi], prior=pw[lo:hi])
                res[r] = e.fit_glm_nb(lnk, **kw)
                assert e.get_theta() == res[r].theta
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    comm.close()
    assert not errs, errs
    for r in range(2):
        check_fit(f"glm.nb local rank {r}", res[r].fit, c["ref"].fit, cond)
        assert abs(res[r].theta - c["ref"].theta) <= 1e-9 * c["ref"].theta
    # every rank holds the same bits
    assert np.array_equal(res[0].fit.coefs, res[1].fit.coefs)
    assert (res[0].theta, res[0].twologlik) == (res[1].theta, res[1].twologlik)


# ---- 6. inference on a negative binomial fit ----
def _c_bar(cond):
    return max(1e-9, K_BOUND * cond * EPS)


def test_inference_on_a_negbin_fit():
    n, p, theta, lnk = 6001, 70, 3.0, "log"
    c = _ref(lnk, n, p, theta)
    X, y, off, pw, beta = c["X"], c["y"], c["off"], c["pr"], c["fits"]["single"].coefs
    eta = X @ beta + off
    mu = np.exp(eta)
    g, v = 1.0 / mu, NB.variance(mu, theta)
    w = pw / (v * g * g)
    Q, Rf = np.linalg.qr(np.sqrt(w)[:, None] * X)
    h = np.sum(Q * Q, axis=1)
    Ri = np.linalg.inv(Rf)
    C = Ri @ Ri.T
    e_, s = y - mu, np.abs(y) + np.abs(mu)
    sp = np.sqrt(pw / v)
    ref = dict(w=w, h=h, mu=mu, e=e_, s=s, pw=pw,
               res={"response": (e_, s), "working": (e_ * g, s * np.abs(g)), "pearson": (e_ * sp, s * sp),
                    "deviance": (np.sign(e_) * 2.0 * NB.dev_rows(y, mu, pw, theta), s)})
    u = w * e_ * g
    assert h.max() <= 0.5
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        e.set_theta(theta)
        cond = gram_cond(e, beta, "negbin", lnk)
        cov = e.vcov(beta, "negbin", lnk)
        err = scaled_err(cov, C)
        print(f"\nMARGIN negbin vcov: {_c_bar(cond) / max(err, 1e-300):.3g}")
        assert err <= _c_bar(cond)
        for kind in ("response", "working", "pearson", "deviance"):
            inf = e.influence(beta, "negbin", lnk, resid=kind)
            check_resid("negbin/log", kind, inf.resid, ref)
        check_hat("negbin/log", inf.hat, ref, cond)
        assert abs(inf.sum_hat - p) <= 1e-9 * p
        # HC3
        omega = u * u / (1.0 - h) ** 2
        M = X.T @ (omega[:, None] * X)
        V = C @ M @ C
        V = 0.5 * (V + V.T)
        amp = h_amp(h, "HC3")
        Vg, Mg = e.vcov_robust(beta, "negbin", lnk, type="HC3", return_meat=True)
        e_v, e_m = scaled_err(Vg, V), scaled_err(Mg, M)
        bar_v, bar_m = _c_bar(cond) * (2.0 + amp), 1e-9 * (1.0 + amp)
        print(f"MARGIN negbin HC3: {min(bar_v / max(e_v, 1e-300), bar_m / max(e_m, 1e-300)):.3g}")
        assert e_v <= bar_v and e_m <= bar_m
        # 40 clusters (vcovCL's defaults: HC1, cadjust)
        G = 40
        ids = np.random.default_rng(3).integers(0, G, n)
        S = np.zeros((G, p))
        np.add.at(S, ids, u[:, None] * X)
        Mc = S.T @ S
        Vc = C @ Mc @ C
        Vc = 0.5 * (Vc + Vc.T) * ((n - 1.0) / (n - p)) * (G / (G - 1.0))
        e.set_clusters(ids, G)
        Vg, Mg = e.vcov_cluster(beta, "negbin", lnk, return_meat=True)
        e_v, e_m = scaled_err(Vg, Vc), scaled_err(Mg, Mc)
        print(f"MARGIN negbin cluster: {min(2 * _c_bar(cond) / max(e_v, 1e-300), 1e-9 / max(e_m, 1e-300)):.3g}")
        assert e_v <= 2 * _c_bar(cond) and e_m <= 1e-9
        # predictions
        assert rel(e.predict_glm(beta, "negbin", lnk, "response"), mu) < 1e-13
        assert rel(e.predict_new(X[:500], beta, "negbin", lnk, "response", offset=off[:500]), mu[:500]) < 1e-13


def test_glm_fit_nb_python_api():
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    n, p = 3001, 6
    X, y, off, pw, _ = NB.make_case("log", n, p, 2.0, 77)
    names = [f"x{j}" for j in range(p)]
    xf, yf = Frame({nm: X[:, j] for j, nm in enumerate(names)}), Frame({"y": y})
    of, pf = Frame({"o": off}), Frame({"w": pw})
    o = NB.glm_nb(X, y, "log", offset=off, prior=pw)
    m = GLM.fit_nb(yf, xf, offset=of, prior=pf)
    assert (m.family, m.link) == ("negbin", "log")
    # (the defaults' stopping decisions are not vetted here as the parity tests' are: loose bars)
    assert abs(m.theta - o.theta) <= 1e-5 * o.theta and abs(m.theta_se - o.se_theta) <= 1e-4 * o.se_theta
    assert rel(m.coefs.reshape(-1), o.fit.coefs) < 1e-5
    assert abs(m.aic - (-m.twologlik + 2 * (p + 1))) <= 1e-12 * abs(m.twologlik)   # theta counts as a parameter
    assert abs(m.twologlik - o.twologlik) <= 1e-8 * abs(o.twologlik)
    text = GLM.summary_string(m)
    assert "Theta: " in text and "Family: negbin" in text
    V = GLM.vcov(m, yf, xf, offset=of, prior=pf)
    assert rel(np.sqrt(np.diag(V)), np.asarray(m.stdErr)) < 1e-3  # (the fit's are the last solve's, one step behind)
    assert GLM.coeftest(m, yf, xf, offset=of, prior=pf).columns == ["name", "estimate", "se", "stat", "pvalue"]
    inf = GLM.influence(m, yf, xf, offset=of, prior=pf)
    assert abs(inf.sum_hat - p) <= 1e-9 * p
    pred = m.predict(xf, offset=of)
    assert rel(pred["value"], np.exp(X @ m.coefs.reshape(-1) + off)) < 1e-12
    fixed = GLM.fit_nb(yf, xf, theta=2.0, offset=of, prior=pf)
    want = NB.fit_glm(X, y, 2.0, "log", offset=off, prior=pw)
    assert fixed.theta == 2.0 and fixed.theta_se is None
    assert rel(fixed.coefs.reshape(-1), want.coefs) < 1e-5
    assert abs(fixed.aic - (-2 * fixed.loglik + 2 * p)) <= 1e-12 * abs(fixed.loglik)
    assert abs(fixed.loglik - want.loglik) <= 1e-8 * abs(want.loglik)


@pytest.mark.parametrize("bad", [-1e30, -3.5, float("nan"), float("inf"), -9.5e15])
def test_a_y_outside_the_counts_domain_is_an_error_not_a_long_kernel(bad):
    """A negative or non-finite y (a missing-value sentinel): the row's theta terms are NaN -- every loop of the
    kernel is bounded whatever the data -- and the calls that estimate from them return SGLM_EINVAL."""
    n, p = 3001, 5
    X, y, off, pw, beta = NB.make_case("log", n, p, 2.0, 7)
    y = y.copy()
    y[1234] = bad
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        t = e.theta_terms(beta, 2.0)
        assert np.isnan(t[0]) and np.isnan(t[1]) and np.isfinite(t[4])
        with pytest.raises(L.IllegalArgumentException, match="theta.ml"):
            e.theta_ml(beta)
        with pytest.raises(L.IllegalArgumentException):
            e.fit_glm_nb("log")
        y[1234] = 2.0   # the handle stays usable
        e.set_data(X, y, offset=off, prior=pw)
        assert np.all(np.isfinite(e.theta_terms(beta, 2.0)))
