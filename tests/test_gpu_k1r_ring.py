"""K1r's buffer ring at 16 column blocks (p = 241..256) against K1 (SGLM_FUSED_SPLIT=0), bitwise, at
the smallest shards where the ring's hand-offs can go wrong: the LDS-DMA of a block is issued by
Gram waves 0..3 once every wave is done with the slot's previous block, the row waves wait for it
to land, the Gram waves for the row stage (per-slot counters landed / ready / done, fused.hpp
pass_body_r).

Rows: 16 and 17 (half a row block, and one row past it: the rest of the block is masked), 47 (a
ragged second block), 5 000 (fewer blocks than workgroups: most workgroups run no block at all),
24 589 (about three blocks per workgroup: both slots are reused once, the last block ragged) and
65 551 (several reuses: the counters' rounds advance).  p = 256 and p = 242 (column quads past p
are duplicates in the LDS image).  Poisson / log with offset and prior weights stages all four
row vectors; the binomial case with group sizes comes from the host (the device generator's group
sizes are all one).  A fit also runs the initial pass, and its deviance-only passes run the ring
without the Gram."""
import os

import numpy as np
import pytest

from sparkglm_amd import Engine

pytestmark = pytest.mark.gpu

ROWS = [16, 17, 47, 5_000, 24_589, 65_551]


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
    assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _check_pass_and_fit(load, p, family, link, beta, fit=True):
    def run(e):
        g, xz, s = e.irls_pass(beta, family=family, link=link)
        f = e.fit_glm(family, link) if fit else None
        return g, xz, s, f, e.stats()["dev_passes"]

    (g0, xz0, s0, f0, d0), (g1, xz1, s1, f1, d1) = _both(load, run)
    _same(g0, g1, "X'WX")
    _same(xz0, xz1, "X'Wz")
    _same(s0, s1, "deviance, sum of weights")
    if fit:
        assert f0.iter == f1.iter and d0 == d1
        _same(f0.coefs, f1.coefs, "coefficients")
        _same(f0.stderr, f1.stderr, "standard errors")
        # (equal_nan: the log-likelihood of proportions y = k / m is NaN under either kernel)
        assert np.array_equal([f0.deviance, f0.null_deviance, f0.pearson, f0.loglik],
                              [f1.deviance, f1.null_deviance, f1.pearson, f1.loglik], equal_nan=True)
    return d1


@pytest.mark.parametrize("p", [256, 242])
@pytest.mark.parametrize("n", ROWS)
def test_poisson_offset_prior_bitwise_k1(n, p):
    beta = np.random.default_rng(n + p).normal(0.0, 0.02, p)
    # a fit needs more rows than columns
    _check_pass_and_fit(lambda e: e.synth(2, 0, n, p, 11), p, "poisson", "log", beta, fit=n > 2 * p)


def test_binomial_group_sizes_bitwise_k1():
    n, p = 5_000, 256
    rng = np.random.default_rng(7)
    X = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, p)) / np.sqrt(p))
    X[:, 0] = 1.0
    m = rng.integers(1, 6, n).astype(np.float64)
    y = rng.binomial(m.astype(np.int64), 0.4) / m
    beta = rng.normal(0.0, 0.02, p)
    _check_pass_and_fit(lambda e: e.set_data(X, y, m=m), p, "binomial", "logit", beta)


def test_deviance_only_passes_bitwise_k1():
    """A fit that ends with deviance-only passes (no Gram): the ring runs with the MFMA waves idle."""
    n, p = 24_589, 256
    beta = np.random.default_rng(3).normal(0.0, 0.02, p)
    dev_passes = _check_pass_and_fit(lambda e: e.synth(0, 0, n, p, 11), p, "binomial", "logit", beta)
    assert dev_passes >= 1


@pytest.mark.parametrize("n", [17, 24_589])
def test_initial_pass_bitwise_k1(n):
    """irls_pass(None, mu0): binomial takes the fast initial row, Poisson the general one."""
    for kind, family, link, mu0 in ((0, "binomial", "logit", 0.3), (2, "poisson", "log", 1.7)):
        (a, b) = _both(lambda e: e.synth(kind, 0, n, 256, 5), lambda e: e.irls_pass(None, mu0=mu0, family=family, link=link))
        for x, y, what in zip(a, b, ("X'WX", "X'Wz", "scalars")):
            _same(x, y, f"{family} {what}")


@pytest.mark.parametrize("n", [47, 24_589])
def test_gaussian_lm_gram_bitwise_k1(n):
    def run(e):
        g, xz, s = e.irls_pass(np.zeros(256), family="gaussian", link="identity")
        f = e.fit_lm() if n > 512 else None
        return g, xz, s, f

    (g0, xz0, s0, f0), (g1, xz1, s1, f1) = _both(lambda e: e.synth(1, 0, n, 256, 9), run)
    _same(g0, g1, "X'X")
    _same(xz0, xz1, "X'y")
    _same(s0, s1, "scalars")
    if f0 is not None:
        _same(f0.coefs, f1.coefs, "coefficients")
        _same(f0.stderr, f1.stderr, "standard errors")
        assert (f0.sse, f0.r2) == (f1.sse, f1.r2)
