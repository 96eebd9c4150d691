"""The cluster-robust covariance's interface without a GPU: the engine's segmentation rule
(sglm_cluster_plan) against its numpy restatement, the argument checks of the C ABI and of the Python
layer, and the identities of the numpy reference (tests/cluster_reference.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cluster_reference as CR
from sandwich_reference import sandwich, scaled_err
from sparkglm_amd import _lib as L
from sparkglm_amd import synth
from sparkglm_amd.engine import Engine, glm_opts
from sparkglm_amd.frame import Frame
from sparkglm_amd.glm import GLM, GLMModel
from sparkglm_amd.lm import LM, LMModel


def tile_rows():
    return L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0]


def test_new_symbols_are_exported():
    for s in ("sglm_set_clusters", "sglm_vcov_cluster", "sglm_get_cluster_ms", "sglm_cluster_plan"):
        assert s in L.EXPORTS and hasattr(L.load(), s)
    assert L.CLUSTER_TYPES == ("HC0", "HC1")


@pytest.mark.parametrize("pattern", CR.PATTERNS)
def test_plan_matches_the_rule(pattern):
    T = tile_rows()
    assert T >= 32 and T % 32 == 0
    for n in (1, T - 1, T, T + 1, 2 * T + 1000, 5 * T + 244 + 3 * 37 + 5):
        ids, G = CR.make_ids(pattern, n, T)
        t, start, clus = L.cluster_plan(ids, G)
        want_start, want_clus = CR.segments(ids, T)
        assert t == T
        assert np.array_equal(start, want_start) and np.array_equal(clus, want_clus), (pattern, n)
        # the segments tile [0, n) exactly, each holds one id and lies within one tile
        assert start[0] == 0 and start[-1] == n and np.all(np.diff(start) > 0)
        for k in range(len(clus)):
            lo, hi = start[k], start[k + 1]
            assert np.all(ids[lo:hi] == clus[k]) and lo // T == (hi - 1) // T
        runs = 1 + int(np.count_nonzero(ids[1:] != ids[:-1]))
        assert len(clus) <= runs + -(-n // T)
    if pattern == "singletons":
        assert len(clus) == n
    if pattern == "sorted":  # the usual panel layout: about G + n / T segments
        assert len(clus) <= G + -(-n // T)


def test_plan_edge_cases():
    lib = L.load()
    t, start, clus = L.cluster_plan(np.zeros(0, dtype=np.int32), 3)
    assert np.array_equal(start, [0]) and len(clus) == 0  # n = 0
    ids = np.array([0, 1, 2, 3], dtype=np.int32)
    ip = ids.ctypes.data_as(C.POINTER(C.c_int32))
    nseg = C.c_int64()
    assert lib.sglm_cluster_plan(ip, 4, 3, None, C.byref(nseg), None, None) == L.SGLM_EINVAL  # id >= G
    assert "[0, G = 3)" in L.last_error()
    ids[3] = -1
    assert lib.sglm_cluster_plan(ip, 4, 4, None, C.byref(nseg), None, None) == L.SGLM_EINVAL
    assert lib.sglm_cluster_plan(None, 4, 4, None, C.byref(nseg), None, None) == L.SGLM_EINVAL
    ids[3] = 3
    assert lib.sglm_cluster_plan(ip, 4, 4, None, C.byref(nseg), None, None) == L.SGLM_OK and nseg.value == 4
    with pytest.raises(L.IllegalArgumentException):
        L.cluster_plan([0, 5], 5)


def test_c_abi_argument_checks():
    lib = L.load()
    o = glm_opts("binomial", "logit")
    b, c = np.zeros(3), np.zeros((3, 3), order="F")
    call = lambda h, hc, cadj=1: lib.sglm_vcov_cluster(h, C.byref(o), L.ptr(b), hc, cadj, c.ctypes.data_as(L.dp), None)
    for hc in (2, 3, -1, 4):  # HC2 / HC3 need per-cluster leverage blocks
        assert call(None, hc) == L.SGLM_EINVAL
        assert "SGLM_HC0 or SGLM_HC1" in L.last_error()
    assert call(None, 1) == L.SGLM_EINVAL and "null engine handle" in L.last_error()
    assert lib.sglm_vcov_cluster(None, None, L.ptr(b), 0, 0, c.ctypes.data_as(L.dp), None) == L.SGLM_EINVAL
    assert lib.sglm_vcov_cluster(None, C.byref(o), L.ptr(b), 0, 0, None, None) == L.SGLM_EINVAL
    ids = np.zeros(3, dtype=np.int32)
    assert lib.sglm_set_clusters(None, ids.ctypes.data_as(C.POINTER(C.c_int32)), 3, 1) == L.SGLM_EINVAL
    t = [C.c_double() for _ in range(4)]
    assert lib.sglm_get_cluster_ms(None, *[C.byref(v) for v in t]) == L.SGLM_EINVAL


def test_python_refuses_the_other_types_before_any_library_call():
    e = Engine.__new__(Engine)  # no device, no library handle: the refusal must come first
    e.n, e.p, e._h = 4, 3, None
    for t in ("const", "HC2", "HC3", "HC4"):
        with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
            e.vcov_cluster(np.zeros(3), type=t)
    obj = GLMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 1.0, 1.0, 1.0, 2.5, 1.0, 0.0, "gaussian", "identity",
                   0.0, 1, 2.0, 1)
    lm = LMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 0.5, 2.0, 3.0, 1)
    fr, cl = Frame({"a": np.ones(3)}), Frame({"id": np.array(["u", "v", "u"])})
    for t in ("const", "HC2", "HC3"):
        with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
            GLM.vcov_cluster(obj, fr, fr, cl, type=t)
        with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
            GLM.coeftest(obj, fr, fr, type=t, cluster=cl)
        with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
            LM.vcov_cluster(lm, fr, fr, cl, type=t)
        with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
            LM.coeftest(lm, fr, fr, type=t, cluster=cl)
    with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
        GLM.coeftest(obj, fr, fr, cluster=cl)  # the unchanged default HC3
    with pytest.raises(L.IllegalArgumentException, match=r"\['HC0', 'HC1'\]"):
        LM.coeftest(lm, fr, fr, cluster=cl)


def test_signatures_and_defaults():
    sig = inspect.signature(Engine.vcov_cluster).parameters
    assert list(sig) == ["self", "beta", "family", "link", "type", "cadjust", "return_meat"]
    assert sig["type"].default == "HC1" and sig["cadjust"].default is True and sig["return_meat"].default is False
    assert list(inspect.signature(Engine.set_clusters).parameters) == ["self", "ids", "G"]
    for fn in (GLM.coeftest, LM.coeftest):
        sig = inspect.signature(fn).parameters
        assert sig["cluster"].default is None and sig["cadjust"].default is True and sig["type"].default == "HC3"
    for fn in (GLM.vcov_cluster, LM.vcov_cluster):
        sig = inspect.signature(fn).parameters
        assert sig["type"].default == "HC1" and sig["cadjust"].default is True
    assert callable(Engine.cluster_ms)


class FakeEngine:
    """Stands in for the device: records what the API asks for."""
    V = np.array([[4.0, 0.5], [0.5, 0.25]])

    def __init__(self):
        self.calls = []

    def set_data(self, *a, **k):
        self.calls.append(("set_data", a[0].shape))

    def set_clusters(self, ids, G=None):
        self.calls.append(("set_clusters", list(ids), G))

    def vcov_cluster(self, beta, fam, lnk, type="HC1", cadjust=True, return_meat=False):
        self.calls.append(("vcov_cluster", fam, lnk, type, cadjust))
        return self.V


def test_coeftest_routes_clusters_and_keeps_its_statistics(monkeypatch):
    from scipy import stats
    from sparkglm_amd import glm as G
    from sparkglm_amd import lm as M
    fake = FakeEngine()
    monkeypatch.setattr(G, "_engine", lambda device=0: fake)
    monkeypatch.setattr(M, "_engine", lambda device=0: fake)
    xf = Frame({"a": np.arange(6.0), "b": np.ones(6)})
    yf = Frame({"y": np.array([0.0, 1.0, 0.0, 1.0, 1.0, 0.0])})
    cl = Frame({"firm": np.array(["x", "y", "x", "z", "z", "y"])})
    coefs = np.array([[1.5], [-0.2]])
    se = np.array([2.0, 0.5])
    obj = GLMModel(["a", "b"], "y", coefs, [0.1, 0.2], 8.0, 9.0, 1.0, 2.0, 1.3, 1.0, -1.0, "binomial", "logit", 3.0, 2,
                   6.0, 1)
    t = GLM.coeftest(obj, yf, xf, type="HC1", cluster=cl)
    assert fake.calls[-2] == ("set_clusters", ["x", "y", "x", "z", "z", "y"], None)
    assert fake.calls[-1] == ("vcov_cluster", "binomial", "logit", "HC1", True)
    assert np.array_equal(t["se"], se) and np.array_equal(t["stat"], coefs.reshape(-1) / se)
    assert np.allclose(t["pvalue"], 2.0 * stats.norm.sf(np.abs(t["stat"])), rtol=0, atol=1e-12)  # z, as without
    assert GLM.vcov_cluster(obj, yf, xf, cl, type="HC0", cadjust=False) is fake.V
    assert fake.calls[-1] == ("vcov_cluster", "binomial", "logit", "HC0", False)
    lm = LMModel(["a", "b"], "y", coefs, [0.1, 0.2], 0.5, 0.9, 2.0, 6.0, 1)
    t = LM.coeftest(lm, xf, yf, type="HC0", cluster=cl, cadjust=False)
    assert fake.calls[-1] == ("vcov_cluster", "gaussian", "identity", "HC0", False)
    assert np.allclose(t["pvalue"], 2.0 * stats.t.sf(np.abs(t["stat"]), 6 - 2), rtol=0, atol=1e-12)  # t on n - p
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        GLM.vcov_cluster(obj, yf, xf, Frame({"firm": np.arange(5)}))
    with pytest.raises(L.IllegalArgumentException, match="only one column"):
        LM.vcov_cluster(lm, xf, yf, Frame({"f": np.arange(6), "g": np.arange(6)}))


@pytest.fixture(scope="module")
def logit_case():
    n, p = 3001, 20
    X, y, _, _ = synth.generate(0, 0, n, p, 7 + p)
    beta = np.zeros(p)
    for _ in range(3):  # three IRLS iterations
        mu = 1.0 / (1.0 + np.exp(-(X @ beta)))
        w = mu * (1.0 - mu)
        beta = np.linalg.solve(X.T @ (w[:, None] * X), X.T @ (w * (X @ beta) + (y - mu)))
    return X, y, beta


def test_reference_singletons_give_the_hc0_meat(logit_case):
    X, y, beta = logit_case
    n = len(y)
    ref = CR.cluster_cov(X, y, beta, "binomial", "logit", np.arange(n), n, "HC0", False)
    hc0 = sandwich(X, y, beta, "binomial", "logit", "HC0")
    assert scaled_err(ref["M"], hc0["M"]) <= 1e-13
    assert scaled_err(ref["V"], hc0["V"]) <= 1e-13


def test_reference_is_invariant_under_a_row_permutation(logit_case):
    X, y, beta = logit_case
    n = len(y)
    T = tile_rows()
    for pattern in ("sorted", "interleaved", "two_level"):
        ids, G = CR.make_ids(pattern, n, T)
        a = CR.cluster_cov(X, y, beta, "binomial", "logit", ids, G)
        perm = np.random.default_rng(3).permutation(n)
        b = CR.cluster_cov(X[perm], y[perm], beta, "binomial", "logit", ids[perm], G)
        assert scaled_err(b["M"], a["M"]) <= 1e-13, pattern
        # the reference's own error: extended precision, and the rows summed in reverse order
        c = CR.cluster_cov(X, y, beta, "binomial", "logit", ids, G, dtype=np.longdouble)
        d = CR.cluster_cov(X, y, beta, "binomial", "logit", ids, G, reverse=True)
        assert scaled_err(c["M"], a["M"]) <= 1e-13 and scaled_err(d["M"], a["M"]) <= 1e-13, pattern
        assert scaled_err(c["V"], a["V"]) <= 1e-13 and scaled_err(d["V"], a["V"]) <= 1e-13, pattern
        dg = np.diag(a["M"])
        assert dg.min() / dg.max() >= 1e-4  # the scaled metric is not degenerate


def test_reference_adjustments():
    assert CR.adjustment(100, 5, 10, "HC0", False) == 1.0
    assert CR.adjustment(100, 5, 10, "HC1", False) == 99.0 / 95.0  # vcovCL's n - 1, not vcovHC's n
    assert CR.adjustment(100, 5, 10, "HC0", True) == 10.0 / 9.0
    assert CR.adjustment(100, 5, 10, "HC1", True) == (99.0 / 95.0) * (10.0 / 9.0)
