"""K1r's row stage at 16 column blocks (p = 241..256) against K1 (SGLM_FUSED_SPLIT=0), bitwise, on the
rows where the row stage itself branches (fused.hpp row_stage_r): its lanes keep the 32 betas of their
column group in registers, and store w, w*z and eta and bump `ready` before the logit fast path's unit
deviance is formed -- the deviance of such a row is added after the hand-off, the deviance of a row on
the reference path before it, in the same wave.

What tests/test_gpu_k1r_ring.py does not reach:
  * binomial / logit rows with |eta| >= 8 (reference path) and |eta| < 8 (fast path) inside the same
    8-row group of a row wave, and a few y outside [0, 1] (reference path too), at p = 256 and 242;
    the pass outputs, and -- through a one-iteration fit started at the same beta, whose Pearson
    statistic and log-likelihood are formed from the eta the pass stored -- the stored eta;
  * prior weights of zero mixed in (Poisson / log with offset);
  * a non-canonical pair and gamma / inverse: other branches of the row stage;
  * the initial pass, a fit's deviance-only passes and the LM Gram, whose rows defer nothing: the sums
    must be complete when the epilogue adds them.  (A deviance-only pass runs inside a fit only, which
    needs more rows than columns: 24 589 rows, not 17.)

Rows: 17 and 47 (one and two ragged blocks) and 24 589 (about three blocks per workgroup: both ring
slots reused, the last block ragged)."""
import os

import numpy as np
import pytest

from sparkglm_amd import Engine

pytestmark = pytest.mark.gpu


def _engine(split: bool) -> Engine:
    saved = os.environ.get("SGLM_FUSED_SPLIT")
    os.environ["SGLM_FUSED_SPLIT"] = "1" if split else "0"
    try:
        return Engine(0)
    finally:
        if saved is None:
            os.environ.pop("SGLM_FUSED_SPLIT", None)
        else:
            os.environ["SGLM_FUSED_SPLIT"] = saved


def _both(load, run):
    """run(engine) under K1 and under K1r on the data load(engine) sets."""
    out = []
    for split in (False, True):
        with _engine(split) as e:
            load(e)
            out.append(run(e))
            assert e.stats()["pass_kernel"] == (2 if split else 1)  # K1r / K1 ran (sglm.h sglm_pass_kernel)
    return out


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what  # bit for bit, NaNs included


def _same_pass(r0, r1, what=""):
    for x, y, name in zip(r0, r1, ("X'WX", "X'Wz", "deviance, sum of weights")):
        _same(x, y, f"{what} {name}")


def _same_fit(f0, f1):
    assert f0.iter == f1.iter
    _same(f0.coefs, f1.coefs, "coefficients")
    _same(f0.stderr, f1.stderr, "standard errors")
    _same([f0.deviance, f0.null_deviance, f0.pearson, f0.loglik], [f1.deviance, f1.null_deviance, f1.pearson, f1.loglik],
          "deviance, null deviance, Pearson, log-likelihood")


def _design(rng, n, p):
    X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, p)))
    X[:, 0] = 1.0
    return X


def _mixed_logit(n, p):
    """X, y, beta with eta = X beta of standard deviation ~6: about a fifth of the rows beyond |eta| = 8."""
    rng = np.random.default_rng(1000 * p + n)
    X = _design(rng, n, p)
    beta = rng.normal(0.0, 6.0 / np.sqrt(p / 3.0), p)
    beta[0] = 0.25
    eta = X @ beta
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    # the host's eta differs from the kernels' by rounding only: rows this far from 8 are on the side they seem
    ref, fast = np.abs(eta) >= 8.5, np.abs(eta) <= 7.5
    k = n // 8 * 8
    both = ref[:k].reshape(-1, 8).any(axis=1) & fast[:k].reshape(-1, 8).any(axis=1)
    assert both.sum() >= max(1, k // 8 // 4), "8-row groups with rows on both paths"
    return X, y, beta


@pytest.mark.parametrize("p", [256, 242])
@pytest.mark.parametrize("n", [47, 24_589])
def test_binomial_mixed_lanes_bitwise_k1(n, p):
    X, y, beta = _mixed_logit(n, p)
    y_out = y.copy()
    y_out[[1, 5, n // 2, n - 2]] = [1.5, -0.25, 2.0, -1.0]  # outside [0, 1]: the reference path, beside fast rows

    r0, r1 = _both(lambda e: e.set_data(X, y_out), lambda e: e.irls_pass(beta))
    _same_pass(r0, r1, "y outside [0, 1]:")

    def run(e):
        r = e.irls_pass(beta)
        # one IRLS pass at beta, then the final statistics from the eta that pass stored
        f = e.fit_glm("binomial", "logit", max_iter=1, start=beta) if n > 2 * p else None
        return r, f

    (r0, f0), (r1, f1) = _both(lambda e: e.set_data(X, y), run)
    _same_pass(r0, r1)
    if f0 is not None:
        _same_fit(f0, f1)


@pytest.mark.parametrize("n", [47, 24_589])
def test_poisson_zero_prior_weights_bitwise_k1(n):
    p = 256
    rng = np.random.default_rng(n)
    X = _design(rng, n, p) / np.sqrt(p)
    X[:, 0] = 1.0
    beta = rng.normal(0.0, 0.3, p)
    off = rng.uniform(-0.5, 0.5, n)
    y = rng.poisson(np.exp(X @ beta + off)).astype(np.float64)
    prior = rng.uniform(0.5, 2.0, n)
    prior[rng.uniform(size=n) < 0.25] = 0.0
    prior[:3] = [0.0, 1.0, 0.0]

    def run(e):
        r = e.irls_pass(beta, family="poisson", link="log")
        f = e.fit_glm("poisson", "log") if n > 2 * p else None
        return r, f

    (r0, f0), (r1, f1) = _both(lambda e: e.set_data(X, y, offset=off, prior=prior), run)
    _same_pass(r0, r1)
    if f0 is not None:
        _same_fit(f0, f1)


@pytest.mark.parametrize("family,link", [("poisson", "sqrt"), ("gamma", "inverse")])
def test_other_row_branches_bitwise_k1(family, link):
    n, p = 24_589, 256
    rng = np.random.default_rng(len(family) + 31 * len(link))
    X = _design(rng, n, p) / np.sqrt(p)
    X[:, 0] = 1.0
    beta = rng.normal(0.0, 0.1, p)
    beta[0] = 1.5  # eta in about 1.5 +- 0.3: positive, as both links need
    eta = X @ beta
    assert eta.min() > 0.5
    y = rng.poisson(eta * eta).astype(np.float64) if family == "poisson" else rng.gamma(2.0, 0.5 / eta)
    y[7] = 0.0  # gamma: outside the fast path's range (the reference order)

    def run(e):
        return e.irls_pass(beta, family=family, link=link), e.irls_pass(None, mu0=1.3, family=family, link=link)

    (a0, i0), (a1, i1) = _both(lambda e: e.set_data(X, y), run)
    _same_pass(a0, a1, f"{family}/{link}")
    _same_pass(i0, i1, f"{family}/{link} initial pass")


@pytest.mark.parametrize("n", [17, 24_589])
def test_initial_pass_and_lm_gram_bitwise_k1(n):
    """Passes whose rows defer nothing, at 16 column blocks with the deferring row stage compiled in."""
    for kind, family, link, mu0 in ((0, "binomial", "logit", 0.3), (2, "poisson", "log", 1.7)):
        a, b = _both(lambda e: e.synth(kind, 0, n, 256, 5), lambda e: e.irls_pass(None, mu0=mu0, family=family, link=link))
        _same_pass(a, b, f"{family} initial pass")

    def run(e):
        r = e.irls_pass(np.zeros(256), family="gaussian", link="identity")
        return r, (e.fit_lm() if n > 512 else None)

    (r0, f0), (r1, f1) = _both(lambda e: e.synth(1, 0, n, 256, 9), run)
    _same_pass(r0, r1, "LM Gram")
    if f0 is not None:
        _same(f0.coefs, f1.coefs, "coefficients")
        _same(f0.stderr, f1.stderr, "standard errors")
        assert (f0.sse, f0.r2) == (f1.sse, f1.r2)


def test_deviance_only_passes_after_deferred_rows_bitwise_k1():
    """A whole fit on the mixed design: IRLS passes that defer the fast rows' deviance, then deviance-only
    passes (no Gram: the row waves run ahead of nothing) whose sums the epilogue must find complete."""
    n, p = 24_589, 256
    X, y, beta = _mixed_logit(n, p)

    def run(e):
        f = e.fit_glm("binomial", "logit", start=0.05 * beta, max_iter=25)
        return f, e.stats()["dev_passes"]

    (f0, d0), (f1, d1) = _both(lambda e: e.set_data(X, y), run)
    assert d0 == d1 and d1 >= 1
    _same_fit(f0, f1)
