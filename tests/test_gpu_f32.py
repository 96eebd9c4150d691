"""Float32-stored designs (narrow_f32.hip irls_narrow_f32_kernel, p <= 64) against the oracle on the design
rounded to float32: a float widens exactly, so the project's single bar (1e-9, the same iteration count)
applies unchanged.  Entries are scaled by an irrational so that none is a float.  Shapes sit at the kernel's
edges: the DMA column groups (p = 1, 5, 17, 33), T4 (gaussian p <= 20), both block geometries (64 rows at
p <= 32, 32 above), waves with no, one and an odd number of blocks, a ragged last block."""
import threading

import numpy as np
import pytest

from conftest import check_fit, nrel, rel
from sparkglm_amd import Engine, synth
from sparkglm_amd import _lib as L
from sparkglm_amd import distributed as D

pytestmark = pytest.mark.gpu

r32 = lambda X: np.asfortranarray(X.astype(np.float32).astype(np.float64))


def design(kind, n, p, seed):
    X, y, off, pr = synth.generate(kind, 0, n, p, seed)
    X[:, 1:] *= np.sqrt(2.0)  # not floats (column 0 stays the intercept)
    return X, y, off, pr


FITS = [
    # (n, p, synth kind, family, link, extras)
    (37, 1, 0, "binomial", "logit", ""),
    (64 * 8 * 3 + 1, 5, 0, "binomial", "logit", "m"),
    (4099, 16, 0, "binomial", "probit", ""),
    (64 * 8 * 5 - 1, 17, 2, "poisson", "log", "offset+prior"),
    (20011, 20, 1, "gaussian", "identity", ""),
    (4099, 32, 0, "binomial", "logit", ""),
    (20011, 33, 3, "gamma", "inverse", ""),
    (64 * 8 * 2 + 1, 48, 2, "negbin", "log", "theta"),
    (20011, 64, 0, "binomial", "logit", ""),
    (4099, 64, 2, "poisson", "log", "offset+prior"),
]


@pytest.mark.parametrize("n,p,kind,family,link,extras", FITS, ids=[f"{c[0]}x{c[1]}-{c[3]}-{c[5] or 'plain'}" for c in FITS])
def test_fit_matches_the_oracle_on_the_rounded_design(n, p, kind, family, link, extras):
    import pyoracle  # checker only
    X, y, off, pr = design(kind, n, p, 11)
    kw = {}
    if extras == "m":
        kw["m"] = 1.0 + (np.arange(n) % 3)  # y successes of m trials
        y = np.minimum(np.floor(synth.unif(np.arange(n, dtype=np.uint64) + np.uint64(6)) * (kw["m"] + 1.0)), kw["m"])
    if extras == "offset+prior":
        kw.update(offset=off, prior=pr)
    with Engine(0) as e:
        e.set_data(X, y, storage="f32", **kw)
        if family == "negbin":
            e.set_theta(2.0)
        f = e.fit_glm(family, link)
        st = e.stats()
        cond = float(np.linalg.cond(e.irls_pass(f.coefs, family=family, link=link)[0]))
    assert st["pass_kernel_kind"] == "narrow-f32" and st["pass_kernel_name"].startswith("irls_narrow_f32_kernel<")
    if family == "negbin":
        import negbin_reference as nb
        o = nb.fit_glm(r32(X), y, 2.0)
    else:
        o = pyoracle.fit_glm(r32(X), y, family, link, nthreads=8, **kw)
    assert check_fit(f"f32 {n}x{p} {family}", f, o, cond) >= 5.0
    assert rel(f.dev_trace, o.dev_trace) < 1e-9


def test_the_design_really_is_float32():
    import pyoracle
    X, y, _, _ = design(0, 4099, 5, 3)
    o32, o64 = pyoracle.fit_glm(r32(X), y), pyoracle.fit_glm(X, y)
    assert rel(o32.coefs, o64.coefs) > 1e-9  # the rounding is visible at the bar
    with Engine(0) as e:
        f32 = e.set_data(X, y, storage="f32").fit_glm()
        assert e.storage == "f32"
        np.testing.assert_array_equal(e.get_data()[0], r32(X))
        f64 = e.set_data(X, y).fit_glm()
        assert e.storage == "f64"
    assert rel(f32.coefs, f64.coefs) > 1e-9 and rel(f32.coefs, o32.coefs) < 1e-9


def test_get_data_widens_in_row_chunks():
    n, p = 300_001, 64  # n p > 2^24: more than one chunk of the widening scratch, a ragged last one
    X = np.asfortranarray(np.random.default_rng(2).uniform(-1.0, 1.0, (n, p)))
    with Engine(0) as e:
        e.set_data(X, np.zeros(n), storage="f32")
        np.testing.assert_array_equal(e.get_data()[0], r32(X))


@pytest.mark.parametrize("p", [20, 48])
def test_ingest_paths_agree_bitwise(p):
    n = 20011
    X, y, _, _ = synth.generate(0, 0, n, p, 9)
    beta = np.random.default_rng(p).normal(0.0, 0.2, p)
    outs = []
    with Engine(0) as e:
        for load in (lambda: e.set_data(X.astype(np.float32), y, storage="f32"),
                     lambda: e.set_data(X, y).store_f32(),
                     lambda: e.synth(0, 0, n, p, 9, storage="f32")):
            load()
            outs += [e.irls_pass(beta), e.irls_pass(beta)]  # each path, and the pass run twice
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("p", [33, 64])
def test_one_pass_against_the_oracle_partials(p):
    import pyoracle as po
    n = 64 * 8 * 3 + 37
    X, y, _, _ = design(0, n, p, 5)
    beta = np.random.default_rng(p).normal(0.0, 0.2, p)
    with Engine(0) as e:
        G, xz, s = e.set_data(X, y, storage="f32").irls_pass(beta)
    ref = po.shard_partials(r32(X), y, "binomial", "logit", 0, beta)
    tri = p * (p + 1) // 2
    Gr = np.zeros((p, p))
    Gr[np.tril_indices(p)] = ref[:tri]  # row-major lower triangle (driver.cpp unpack_gram)
    Gr = Gr + np.tril(Gr, -1).T
    # the bar of tests/test_gpu_parity.py test_pass_gram_every_kernel_variant
    assert nrel(G, Gr) < 1e-13 and nrel(xz, ref[tri:tri + p]) < 1e-13 and rel(s[0], ref[tri + p]) < 1e-12


REFUSED = {
    "fit_lm": lambda e, p: e.fit_lm(),
    "influence": lambda e, p: e.influence(np.zeros(p)),
    "vcov_robust": lambda e, p: e.vcov_robust(np.zeros(p)),
    "fit_glm_firth": lambda e, p: e.fit_glm_firth(),
    "fit_multinom": lambda e, p: e.fit_multinom(3),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_scope_guard(what):
    X, y, _, _ = design(0, 4099, 5, 7)
    with Engine(0) as e:
        e.set_data(X, y, storage="f32")
        e.reset_stats()
        with pytest.raises(L.IllegalArgumentException, match="fp32"):
            REFUSED[what](e, 5)
        assert e.stats()["passes"] == 0  # refused before any launch
        f = e.fit_glm()
        assert f.iter > 0 and e.stats()["pass_kernel_name"].startswith("irls_narrow_f32_kernel<")


@pytest.mark.parametrize("devices,p", [([0], 65), ([0, 0], 5)], ids=["p65", "group"])
def test_store_f32_refuses_what_it_cannot_hold(devices, p):
    X, y, _, _ = design(0, 1000, p, 7)
    with (Engine(0) if len(devices) == 1 else Engine(devices=devices)) as e:
        e.set_data(X, y)
        with pytest.raises(L.IllegalArgumentException, match="fp32"):
            e.store_f32()
        assert e.fit_glm().iter > 0  # the fp64 data is unchanged


def test_two_ranks_over_the_local_communicator():
    import pyoracle
    n, p = 20011, 33
    X, y, _, _ = design(0, n, p, 13)
    o = pyoracle.fit_glm(r32(X), y, npart=2)
    comm, res, errs = D.LocalComm(2), {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(n, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi], storage="f32")
                res[r] = e.fit_glm(init="multiple", npart=2)
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    assert np.array_equal(res[0].coefs, res[1].coefs) and np.array_equal(res[0].stderr, res[1].stderr)
    assert check_fit("f32 two ranks", res[0], o, 1.0) >= 5.0
