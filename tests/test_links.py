"""The non-canonical links of gaussian, poisson and gamma without a GPU: the numpy reference
(tests/links_reference.py) against np_reference on the canonical pairs and against the likelihood's
score equations, the engine's C++ driver over that reference's partials (sglm_fit_glm_external), the
kernel choice, the Python API's pair table and the out-of-range error path."""
import functools

import numpy as np
import pytest

import links_reference as LR
import np_reference as NR
from conftest import check_fit, rel
from sparkglm_amd import _lib as L
from sparkglm_amd import distributed as D
from sparkglm_amd import synth
from sparkglm_amd.engine import FitGLM, glm_opts


# ---- 1. the reference reproduces np_reference on the six existing pairs ----
def _same_fit(a, b):
    assert a.iter == b.iter
    assert rel(a.coefs, b.coefs) < 1e-12 and rel(a.stderr, b.stderr) < 1e-12
    assert rel([a.deviance, a.null_deviance, a.pearson, a.loglik],
               [b.deviance, b.null_deviance, b.pearson, b.loglik]) < 1e-12


@pytest.mark.parametrize("name", ["logit", "probit", "cloglog", "gaussian", "poisson_offset_prior", "gamma",
                                  "binomial_m_offset", "logit_npart4"])
def test_reference_equals_np_reference_on_golden_cases(golden, name):
    c = golden[name]
    fam, lnk = (str(v) for v in c["meta"][:2])
    kw = {"offset": c.get("offset"), "prior": c.get("prior"), "m": c.get("m")}
    for npart in (1, 4):
        _same_fit(LR.fit_glm(c["X"], c["y"], fam, lnk, npart=npart, **kw),
                  NR.fit_glm(c["X"], c["y"], fam, lnk, npart=npart, **kw))


@pytest.mark.parametrize("kind,fam,lnk", [(0, "binomial", "logit"), (0, "binomial", "probit"),
                                          (0, "binomial", "cloglog"), (1, "gaussian", "identity"),
                                          (2, "poisson", "log"), (3, "gamma", "inverse")])
def test_reference_equals_np_reference_on_synthetic_designs(kind, fam, lnk):
    X, y, off, pr = synth.generate(kind, 0, 2000, 8, 11)
    _same_fit(LR.fit_glm(X, y, fam, lnk, offset=off, prior=pr), NR.fit_glm(X, y, fam, lnk, offset=off, prior=pr))


# ---- 2. the C++ driver over the reference's partials, every new pair ----
@functools.lru_cache(maxsize=None)
def _case(fam, lnk, n, p):
    X, y, off, pr = LR.make_case(fam, n, p)
    traces = [LR.fit_glm(X, y, fam, lnk, offset=off, prior=pr, tol=1e-11, max_iter=40, npart=g).dev_trace
              for g in (1, 2)]
    tol, _ = LR.pick_tol(traces)
    return X, y, off, pr, tol, traces


def _external(X, y, off, pr, fam, lnk, tol, init="single"):
    part = lambda mode, b, mu0, ybar: LR.partials(mode, X, y, fam, lnk, b, mu0, ybar, offset=off, prior=pr)
    return D.fit_glm_external(X.shape[1], lambda: (y.sum(), len(y)), part, family=fam, link=lnk, tol=tol, init=init)


@pytest.mark.parametrize("fam,lnk", LR.NEW_PAIRS)
@pytest.mark.parametrize("n,p", [(3000, 20), (6000, 70)])
def test_driver_over_reference_partials_fits_every_new_pair(fam, lnk, n, p):
    X, y, off, pr, tol, traces = _case(fam, lnk, n, p)
    assert LR.trajectory_ok(traces, tol)
    for init, npart in (("single", 1), ("multiple", 2)):
        o = LR.fit_glm(X, y, fam, lnk, offset=off, prior=pr, tol=tol, npart=npart)
        assert max(o.invalid) == 0
        f = _external(X, y, off, pr, fam, lnk, tol, init)
        check_fit(f"external {fam}/{lnk} {n}x{p} {init}", f, o, LR.gram_cond(X, o, fam, lnk, pr))


# ---- 3. the reference satisfies the likelihood's score equations ----
@pytest.mark.parametrize("fam,lnk", LR.NEW_PAIRS)
@pytest.mark.parametrize("n,p", [(3000, 20), (6000, 70), (6000, 200), (5000, 290)])
def test_reference_fit_solves_the_score_equations(fam, lnk, n, p):
    """X'(pw (y - mu) / (V g')) = 0 at the maximum likelihood estimate, whatever the IRLS details."""
    X, y, off, pr = LR.make_case(fam, n, p)
    tol = 1e-8 if (fam, lnk, p) == ("gaussian", "inverse", 200) else 1e-6
    o = LR.fit_glm(X, y, fam, lnk, offset=off, prior=pr, tol=tol)
    g, v = LR.lprime(fam, lnk, o.mu, 1.0), NR.variance(fam, o.mu, 1.0)
    score = np.max(np.abs(X.T @ (pr * (y - o.mu) / (v * g))))
    scale = np.max(np.abs(X.T @ (pr * np.abs(y) / (v * np.abs(g)))))
    print(f"\nSCORE {fam}/{lnk} {n}x{p}: {score / scale:.2e}")
    assert score <= 1e-6 * scale


# ---- 4. kernel choice ----
@pytest.mark.parametrize("fam,lnk", LR.NEW_PAIRS)
@pytest.mark.parametrize("n,p,fs", [(3001, 16, 1), (3001, 20, 1), (6001, 64, 1), (6001, 70, 1), (6001, 70, 5),
                                    (6001, 150, 1), (6001, 200, 1), (5001, 290, 1)])
def test_new_pairs_run_the_kernel_kind_of_their_canonical_sibling(fam, lnk, n, p, fs):
    kind, name = L.pass_kernel_for(n, p, fam, lnk, fused_split=fs)
    ckind, cname = L.pass_kernel_for(n, p, fam, LR.CANONICAL[fam], fused_split=fs)
    assert kind == ckind and kind in ("narrow", "fused", "fused-split", "wide")
    if kind != "wide":  # the same kernel template and P16; the link slot names the instantiation that runs
        slot = "log" if (fam, lnk) == ("gamma", "log") else "runtime"
        assert name == cname.rsplit(",", 1)[0] + f",{slot}>"


@pytest.mark.parametrize("fam,lnk", [("poisson", "logit"), ("gamma", "sqrt"), ("gaussian", "sqrt"),
                                     ("binomial", "sqrt"), ("binomial", "log")])
def test_other_pairs_are_still_refused(fam, lnk):
    with pytest.raises(L.IllegalArgumentException):
        L.pass_kernel_for(6001, 70, fam, lnk)
    part = lambda *a: np.zeros(2 * 3 // 2 + 2 + L.NS)
    with pytest.raises(L.IllegalArgumentException):
        D.fit_glm_external(2, lambda: (1.0, 2.0), part, family=fam, link=lnk)


def test_sqrt_link_is_part_of_the_abi():
    assert L.LINKS["sqrt"] == 6
    o = glm_opts("poisson", "sqrt")
    assert (o.family, o.link) == (2, 6)


# ---- 5. the Python API ----
def test_python_api_takes_the_pair_table(monkeypatch):
    from sparkglm_amd import glm as G
    from sparkglm_amd.frame import Frame
    seen = []

    class FakeEngine:
        def set_data(self, X, y, m=None, offset=None, prior=None):
            self.p = X.shape[1]

        def fit_glm(self, fam, lnk, **kw):
            seen.append((fam, lnk))
            return FitGLM(np.ones(self.p), np.ones(self.p), 1.0, 2.0, 1.0, -1.0, 3, 6.0, 1)

    monkeypatch.setattr(G, "_engine", lambda device=0: FakeEngine())
    x = Frame({"a": np.ones(6), "b": np.arange(6.0)})
    y = Frame({"y": np.arange(1.0, 7.0)})
    obj = G.GLM.fit(y, x, "gamma", "log")
    assert seen == [("gamma", "log")] and (obj.family, obj.link) == ("gamma", "log")
    G.GLM.fit_weighted(y, x, "Poisson", "sqrt", Frame({"w": np.ones(6)}))
    assert seen[-1] == ("poisson", "sqrt")
    for fam, links in LR.PAIRS.items():
        for lnk in links:
            assert G._engine_family_link(fam, lnk) == (fam, lnk)
    with pytest.raises(L.IllegalArgumentException):
        G.GLM.fit(y, x, "gamma", "sqrt")
    with pytest.raises(L.IllegalArgumentException):
        G.GLM.fit(y, x, "poisson", "logit")
    assert G._engine_family_link("quasi", "sqrt") == ("binomial", "cloglog")  # unknown family: binomial
    eta = np.array([0.2, 0.9, 1.7])
    d = 1e-6
    num = (LR.unlink("poisson", "sqrt", eta + d, 1.0) - LR.unlink("poisson", "sqrt", eta - d, 1.0)) / (2 * d)
    assert np.allclose(G._dmu_deta("sqrt", eta), num, rtol=1e-8)


# ---- 6. a fit that leaves the family's range ----
def test_leaving_the_range_is_an_error_that_names_the_iteration():
    X, y, off, pr = synth.generate(2, 0, 5000, 20, 11)
    o = LR.fit_glm(X, y, "poisson", "identity", offset=off, prior=pr, max_iter=1)
    assert o.invalid[0] == 0 and o.invalid[1] > 0  # the reference alone: rows with mu <= 0 after one step
    with pytest.raises(L.IllegalArgumentException, match="iteration 1"):
        _external(X, y, off, pr, "poisson", "identity", 1e-6)
    # the start: gaussian / log needs mean(y) > 0
    Xg, yg, _, _ = synth.generate(1, 0, 2000, 8, 11)
    yg = yg - yg.mean() - 1.0
    with pytest.raises(L.IllegalArgumentException, match="iteration 0"):
        _external(Xg, yg, None, None, "gaussian", "log", 1e-6)


# ---- 7. the overlapped wide row kernel of the new pairs keeps the canonical kernels' budget ----
def test_new_overlap_row_kernels_fit_beside_the_gram():
    """tests/test_residency.py's budget for the kernels it does not count: at most 96 VGPRs and no
    scratch, so that one such workgroup fits a SIMD beside the two persistent Gram workgroups."""
    from test_residency import _alloc, _kernel_meta
    meta = _kernel_meta()
    rows = {k: v for k, v in meta.items() if "wide_rows_link_ov_kernel" in k}
    assert len(rows) == 3  # one run-time-link instantiation per extension family
    off = meta["_ZN4sglm16wide_gram_kernelILb0ELb0EEEvNS_12WideGramArgsE"]
    for v in rows.values():
        assert v["private_segment_fixed_size"] == 0
        assert _alloc(v["vgpr_count"]) <= 96
        assert 2 * _alloc(off["vgpr_count"]) + _alloc(v["vgpr_count"]) <= 512
