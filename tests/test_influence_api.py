"""The per-row diagnostics' interface without a GPU: argument checks of the new C-ABI calls, the
Python refusals, and GLMModel / LMModel.predict unchanged without a covariance."""
import ctypes as C
import inspect

import numpy as np
import pytest

from sparkglm_amd import _lib as L
from sparkglm_amd.engine import Engine, Influence, glm_opts
from sparkglm_amd.glm import GLMModel, _dispersion, _dmu_deta
from sparkglm_amd.lm import LMModel


def _call_influence(h, opts, disp, rtype=3):
    lib = L.load()
    beta = np.zeros(3)
    return lib.sglm_influence(h, opts, L.ptr(beta), rtype, disp, None, None, None, None)


def test_null_handle_null_opts_and_bad_dispersion_are_einval():
    lib = L.load()
    o = glm_opts("binomial", "logit")
    beta, cov, out = np.zeros(3), np.zeros((3, 3), order="F"), np.zeros(4)
    assert _call_influence(None, C.byref(o), 1.0) == L.SGLM_EINVAL
    assert "null engine handle" in L.last_error()
    assert _call_influence(None, None, 1.0) == L.SGLM_EINVAL
    assert "opts" in L.last_error()
    for disp in (0.0, -1.0, float("nan")):
        assert _call_influence(None, C.byref(o), disp) == L.SGLM_EINVAL
        assert "dispersion > 0" in L.last_error()
    assert _call_influence(None, C.byref(o), 1.0, rtype=4) == L.SGLM_EINVAL
    assert lib.sglm_vcov(None, C.byref(o), L.ptr(beta), cov.ctypes.data_as(L.dp)) == L.SGLM_EINVAL
    assert lib.sglm_predict_new_se(None, L.ptr(out), 1, 3, 1, cov.ctypes.data_as(L.dp), 1.0, L.ptr(out)) == L.SGLM_EINVAL
    ms = C.c_double()
    assert lib.sglm_get_influence_ms(None, C.byref(ms)) == L.SGLM_EINVAL


def test_python_refuses_an_unknown_residual_type():
    e = Engine.__new__(Engine)  # no device: the refusal comes before any library call
    e.n, e.p = 4, 3
    with pytest.raises(L.IllegalArgumentException, match="resid must be one of"):
        e.influence(np.zeros(3), resid="studentized")
    with pytest.raises(L.IllegalArgumentException, match="resid must be one of"):
        e.residuals(np.zeros(3), resid="partial")
    e._h = None
    assert sorted(L.RESID_TYPES) == ["deviance", "pearson", "response", "working"]
    assert [f for f in Influence.__dataclass_fields__] == ["hat", "resid", "cooks", "sum_hat"]


def test_predict_signatures_keep_their_defaults():
    """cov / dispersion / xtxi are optional and default to None: without them predict is today's."""
    sig = inspect.signature(GLMModel.predict).parameters
    assert list(sig)[:6] == ["self", "newData", "type", "offset", "m", "device"]
    assert sig["cov"].default is None and sig["dispersion"].default is None
    sig = inspect.signature(LMModel.predict).parameters
    assert list(sig)[:3] == ["self", "newData", "device"] and sig["xtxi"].default is None


def test_predict_without_cov_returns_the_same_columns(monkeypatch):
    from sparkglm_amd import glm as G
    from sparkglm_amd.frame import Frame

    class FakeEngine:
        def predict_new(self, X, beta, fam, lnk, type, off, m):
            return X @ beta

        def predict_new_se(self, X, cov, phi):
            return np.sqrt(phi * np.einsum("ij,ij->i", X @ cov, X))

    monkeypatch.setattr(G, "_engine", lambda device=0: FakeEngine())
    obj = GLMModel(["a", "b"], "y", np.array([[0.5], [-1.0]]), [0.1, 0.2], 8.0, 9.0, 1.0, 2.0, 1.3, 1.0, -1.0,
                   "gaussian", "identity", 3.0, 2, 10.0, 1)
    new = Frame({"a": np.arange(4.0), "b": np.ones(4)})
    plain = obj.predict(new)
    assert plain.columns == ["index", "value"]
    cov = np.array([[2.0, 0.5], [0.5, 1.0]])
    with_se = obj.predict(new, cov=cov)
    assert with_se.columns == ["index", "value", "se"]
    assert np.array_equal(with_se["value"], plain["value"])
    X = new.to_matrix()
    want = np.sqrt(1.3 * np.einsum("ij,ij->i", X @ cov, X))  # gaussian: the Pearson dispersion (R's rule)
    assert np.allclose(with_se["se"], want, rtol=1e-15)
    assert np.allclose(obj.predict(new, cov=cov, dispersion=4.0)["se"], want * np.sqrt(4.0 / 1.3), rtol=1e-14)


def test_dispersion_rule_and_link_derivatives():
    mk = lambda fam, lnk: GLMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 1.0, 1.0, 1.0, 2.5, 1.0, 0.0, fam, lnk,
                                   0.0, 1, 2.0, 1)
    assert _dispersion(mk("binomial", "logit")) == 1.0 and _dispersion(mk("poisson", "log")) == 1.0
    assert _dispersion(mk("gaussian", "identity")) == 2.5 and _dispersion(mk("Gamma", "inverse")) == 2.5
    # d mu / d eta against a central difference of the oracle's unlink
    import np_reference as R
    eta = np.array([-2.0, -0.3, 0.4, 1.5])
    for fam, lnk, e, m in (("binomial", "logit", eta, 3.0), ("binomial", "probit", eta, 3.0),
                           ("binomial", "cloglog", eta, 3.0), ("gaussian", "identity", eta, 1.0),
                           ("poisson", "log", eta, 1.0), ("gamma", "inverse", np.abs(eta) + 0.5, 1.0)):
        d = 1e-6
        num = (R.unlink(fam, lnk, e + d, m) - R.unlink(fam, lnk, e - d, m)) / (2 * d)
        assert np.allclose(_dmu_deta(lnk, e, m), num, rtol=1e-7), (fam, lnk)
