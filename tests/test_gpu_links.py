"""The non-canonical links of gaussian (log, inverse), poisson (identity, sqrt) and gamma (log, identity)
on every GPU pass path, against the numpy reference tests/links_reference.py (np_reference's IRLS
skeleton with the link functions selected by link).

Shapes: the smallest at which each kernel family can go wrong, n never a multiple of the row blocks --
narrow P16 = 1..4 (p = 20 also the gaussian T4 variant), K1 at 5 and 6 column blocks, K1r at 10 and 13,
K1r at the odd count 5 (SGLM_FUSED_SPLIT=5), the wide path resident and procedural.  Every new pair runs
at one narrow, one K1, one K1r and the wide resident shape; gamma / log (the pair with an inline row
stage) at all of them.

Every case first asserts, of the reference alone, that no row leaves the pair's range at any iteration
and that the stop rule is clear of the trajectory (links_reference.trajectory_ok: the tol of the case
comes from {1e-5, 1e-6, 1e-7, 1e-8}); iteration counts are then compared exactly."""
import functools
import os
import threading

import numpy as np
import pytest

import links_reference as LR
import np_reference as NR
import pyoracle as po
from conftest import check_fit, gram_cond, rel
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D
from test_gpu_influence import check_hat, check_resid

pytestmark = pytest.mark.gpu

ALL = LR.NEW_PAIRS
GL = ("gamma", "log")
# (n, p, SGLM_FUSED_SPLIT or None, kernel kind, pairs)
SHAPES = [
    (3001, 16, None, "narrow", [GL, ("poisson", "sqrt")]),
    (3001, 20, None, "narrow", ALL),
    (4001, 33, None, "narrow", [GL, ("poisson", "identity")]),
    (6001, 64, None, "narrow", [GL, ("gaussian", "log")]),
    (6001, 70, None, "fused", ALL),
    (6001, 96, None, "fused", [GL, ("poisson", "sqrt")]),
    (6001, 150, None, "fused-split", ALL),
    (6001, 200, None, "fused-split", [GL, ("gaussian", "inverse")]),
    (6001, 70, 5, "fused-split", [GL, ("poisson", "identity")]),
    (5001, 290, None, "wide", ALL),
]
CASES = [(n, p, fs, kind, fam, lnk) for n, p, fs, kind, pairs in SHAPES for fam, lnk in pairs]
IDS = [f"{fam}-{lnk}-{n}x{p}{'-split' + str(fs) if fs else ''}" for n, p, fs, kind, fam, lnk in CASES]


def _engine(env=None, devices=None) -> Engine:
    """An engine created under the given SGLM_* settings (they are read at creation)."""
    env = {k: str(v) for k, v in (env or {}).items() if v is not None}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Engine(devices=devices) if devices else Engine(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _ref(fam, lnk, n, p, procedural=False):
    """The inputs of a case and the reference's fits (single and multiple init), computed once."""
    if procedural:
        X, y, _, _ = synth.generate(3, 0, n, p, 11)
        off = pr = None
    else:
        X, y, off, pr = LR.make_case(fam, n, p)
    kw = dict(offset=off, prior=pr)
    traces = [LR.fit_glm(X, y, fam, lnk, tol=1e-11, max_iter=40, npart=g, **kw).dev_trace for g in (1, 2)]
    tol, clear = LR.pick_tol(traces)
    fits = {"single": LR.fit_glm(X, y, fam, lnk, tol=tol, npart=1, **kw),
            "multiple": LR.fit_glm(X, y, fam, lnk, tol=tol, npart=2, **kw)}
    return dict(X=X, y=y, off=off, pr=pr, tol=tol, traces=traces, fits=fits, clear=clear)


def _assert_inputs(c, label):
    """Conditions on the test's inputs (the reference alone), not measurements."""
    for f in c["fits"].values():
        assert max(f.invalid) == 0, (label, f.invalid)
    print(f"\nINPUT {label}: tol {c['tol']:g}, clearance {c['clear']:.1f}, iterations "
          f"{c['fits']['single'].iter} / {c['fits']['multiple'].iter}")
    assert LR.trajectory_ok(c["traces"], c["tol"]), (label, c["tol"], c["clear"])


def _same(a, b):
    assert a.iter == b.iter
    assert np.array_equal(a.coefs, b.coefs) and np.array_equal(a.stderr, b.stderr)
    assert (a.deviance, a.null_deviance, a.pearson, a.loglik) == (b.deviance, b.null_deviance, b.pearson, b.loglik)
    assert np.array_equal(a.dev_trace, b.dev_trace)


@pytest.mark.parametrize("n,p,fs,kind,fam,lnk", CASES, ids=IDS)
def test_fit_on_every_pass_path(n, p, fs, kind, fam, lnk):
    label = f"{fam}/{lnk} {n}x{p}" + (f" split{fs}" if fs else "")
    c = _ref(fam, lnk, n, p)
    _assert_inputs(c, label)
    want_kind, want_name = L.pass_kernel_for(n, p, fam, lnk, fused_split=fs or 1)
    assert want_kind == kind
    fits = {}
    for spec in (1, 0):
        with _engine({"SGLM_FUSED_SPLIT": fs, "SGLM_SPECULATE": spec}) as e:
            e.set_data(c["X"], c["y"], offset=c["off"], prior=c["pr"])
            for init in ("single", "multiple"):
                e.reset_stats()
                f = fits[spec, init] = e.fit_glm(fam, lnk, tol=c["tol"], init=init)
                st = e.stats()
                if spec:
                    assert st["pass_kernel_name"] == want_name and st["pass_kernel_kind"] == kind
                    print(f"PASSES {label} {init}: {st['passes']} passes, {st['dev_passes']} deviance-only, "
                          f"{f.iter} iterations")
                    check_fit(f"{label} {init}", f, c["fits"][init], gram_cond(e, f.coefs, fam, lnk), tol=1e-9)
            if spec:  # one pass twice: bitwise
                a, b = e.irls_pass(f.coefs, family=fam, link=lnk), e.irls_pass(f.coefs, family=fam, link=lnk)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
                assert np.isfinite(a[2][L.S_DEV]) and a[2][L.S_BAD] == 0
    for init in ("single", "multiple"):  # the speculative last pass is bitwise neutral
        _same(fits[1, init], fits[0, init])


@pytest.mark.parametrize("fam,lnk", [GL, ("gaussian", "log")])
def test_procedural_wide_fit(fam, lnk):
    n, p = 6000, 520
    c = _ref(fam, lnk, n, p, procedural=True)
    _assert_inputs(c, f"procedural {fam}/{lnk}")
    with Engine(0) as e:
        e.synth(3, 0, n, p, 11, procedural=True)
        for init in ("single", "multiple"):
            f = e.fit_glm(fam, lnk, tol=c["tol"], init=init)
            assert e.stats()["pass_kernel_kind"] == "wide-procedural"
            check_fit(f"procedural {fam}/{lnk} {init}", f, c["fits"][init], gram_cond(e, f.coefs, fam, lnk))


@pytest.mark.parametrize("fam,lnk", [GL, ("gaussian", "inverse"), ("poisson", "sqrt")])
def test_group_handle_and_two_local_ranks(fam, lnk):
    n, p = 6001, 70
    c = _ref(fam, lnk, n, p)
    _assert_inputs(c, f"multi {fam}/{lnk}")
    X, y, off, pr, o = c["X"], c["y"], c["off"], c["pr"], c["fits"]["multiple"]
    with Engine(0) as one:
        one.set_data(X, y, offset=off, prior=pr)
        cond = gram_cond(one, o.coefs, fam, lnk)
    with Engine(devices=[0]) as g:
        g.set_data(X, y, offset=off, prior=pr)
        check_fit(f"group[0] {fam}/{lnk}", g.fit_glm(fam, lnk, tol=c["tol"], init="multiple"), o, cond)
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(n, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi], offset=off[lo:hi], prior=pr[lo:hi])
                res[r] = e.fit_glm(fam, lnk, tol=c["tol"], init="multiple")
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
        check_fit(f"local rank {r} {fam}/{lnk}", res[r], o, cond)
    assert np.array_equal(res[0].coefs, res[1].coefs)


@pytest.mark.parametrize("fam,lnk", ALL)
def test_prediction_on_the_response_scale(fam, lnk):
    n, p = 3001, 20
    c = _ref(fam, lnk, n, p)
    X, off, beta = c["X"], c["off"], c["fits"]["single"].coefs
    with Engine(0) as e:
        e.set_data(X, c["y"], offset=off, prior=c["pr"])
        want = LR.unlink(fam, lnk, X @ beta + off, 1.0)
        assert rel(e.predict_glm(beta, fam, lnk, "response"), want) < 1e-13
        assert rel(e.predict_glm(beta, fam, lnk, "link"), X @ beta + off) < 1e-13
        Xn = X[:777]
        assert rel(e.predict_new(Xn, beta, fam, lnk, "response", offset=off[:777]), want[:777]) < 1e-13
        assert rel(e.predict_new(Xn, beta, fam, lnk, "response"), LR.unlink(fam, lnk, Xn @ beta, 1.0)) < 1e-13


@pytest.mark.parametrize("fam,lnk", ALL)
def test_influence(fam, lnk):
    """Leverage against a QR of sqrt(w) X and the formula residuals, with test_gpu_influence's bars."""
    n, p = 3001, 20
    c = _ref(fam, lnk, n, p)
    X, y, off, pw, beta = c["X"], c["y"], c["off"], c["pr"], c["fits"]["single"].coefs
    eta = X @ beta + off
    mu = LR.unlink(fam, lnk, eta, 1.0)
    g, v = LR.lprime(fam, lnk, mu, 1.0), NR.variance(fam, mu, 1.0)
    w = pw / (v * g * g)
    Q, _ = np.linalg.qr(np.sqrt(w)[:, None] * X)
    e_, s = y - mu, np.abs(y) + np.abs(mu)
    sp = np.sqrt(pw / v)
    ref = dict(w=w, h=np.sum(Q * Q, axis=1), mu=mu, e=e_, s=s, pw=pw,
               res={"response": (e_, s), "working": (e_ * g, s * np.abs(g)), "pearson": (e_ * sp, s * sp),
                    "deviance": (np.sign(e_) * NR.dev_factor(fam) * NR.dev_rows(fam, y, mu, np.ones(n), pw), s)})
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pw)
        cond = gram_cond(e, beta, fam, lnk)
        for kind in ("response", "working", "pearson", "deviance"):
            inf = e.influence(beta, fam, lnk, resid=kind)
            check_resid(f"{fam}/{lnk}", kind, inf.resid, ref)
            assert np.array_equal(e.residuals(beta, fam, lnk, resid=kind), inf.resid)
        check_hat(f"{fam}/{lnk}", inf.hat, ref, cond)
        assert abs(inf.sum_hat - p) <= 1e-9 * p
        cov = e.vcov(beta, fam, lnk)
        assert rel(np.diag(cov), np.diag(np.linalg.inv((X.T * w) @ X))) < max(1e-9, 20 * cond * np.finfo(float).eps)


def test_leaving_the_range_on_the_device():
    """poisson / identity on the count design of synth kind 2: mu <= 0 after the first step.  NaN
    arithmetic and a status code only; the handle stays usable."""
    X, y, off, pr = synth.generate(2, 0, 5000, 20, 11)
    with Engine(0) as e:
        e.set_data(X, y, offset=off, prior=pr)
        with pytest.raises(L.IllegalArgumentException, match="iteration 1"):
            e.fit_glm("poisson", "identity")
        one = LR.fit_glm(X, y, "poisson", "identity", offset=off, prior=pr, max_iter=1)
        assert one.invalid[1] > 0
        _, _, s = e.irls_pass(one.coefs, family="poisson", link="identity")
        assert (not np.isfinite(s[L.S_DEV])) or s[L.S_BAD] > 0
        with pytest.raises(L.IllegalArgumentException, match="iteration"):
            e.irls_iterations(one.coefs, 1, "poisson", "identity")
        f = e.fit_glm("poisson", "log")
        o = po.fit_glm(X, y, "poisson", "log", offset=off, prior=pr)
        check_fit("poisson/log after the refused fit", f, o, gram_cond(e, f.coefs, "poisson", "log"))
