"""The sandwich covariance's interface without a GPU: argument checks of sglm_vcov_robust /
sglm_get_sandwich_ms, the Python refusals, the signatures, and the coeftest table's arithmetic over a
stand-in engine."""
import ctypes as C
import inspect

import numpy as np
import pytest

from sparkglm_amd import _lib as L
from sparkglm_amd.engine import Engine, glm_opts
from sparkglm_amd.frame import Frame
from sparkglm_amd.glm import GLM, GLMModel
from sparkglm_amd.lm import LM, LMModel


def _call(h, opts, hc, beta=True, cov=True):
    lib = L.load()
    b, c = np.zeros(3), np.zeros((3, 3), order="F")
    return lib.sglm_vcov_robust(h, opts, L.ptr(b) if beta else None, hc, c.ctypes.data_as(L.dp) if cov else None, None)


def test_bad_arguments_are_einval():
    lib = L.load()
    o = glm_opts("binomial", "logit")
    assert _call(None, C.byref(o), 3) == L.SGLM_EINVAL
    assert "null engine handle" in L.last_error()
    assert _call(None, None, 3) == L.SGLM_EINVAL
    assert "opts" in L.last_error()
    for hc in (-1, 4, 17):
        assert _call(None, C.byref(o), hc) == L.SGLM_EINVAL
        assert "hc_type" in L.last_error() and "SGLM_HC3" in L.last_error()
    assert _call(None, C.byref(o), 0, cov=False) == L.SGLM_EINVAL
    assert "cov" in L.last_error()
    assert _call(None, C.byref(o), 0, beta=False) == L.SGLM_EINVAL
    assert "beta" in L.last_error()
    a, b = C.c_double(), C.c_double()
    assert lib.sglm_get_sandwich_ms(None, C.byref(a), C.byref(b)) == L.SGLM_EINVAL
    assert "null engine handle" in L.last_error()


def test_hc_types_follow_the_header():
    assert L.HC_TYPES == {"HC0": 0, "HC1": 1, "HC2": 2, "HC3": 3}
    assert "sglm_vcov_robust" in L.EXPORTS and "sglm_get_sandwich_ms" in L.EXPORTS


def test_python_refuses_an_unknown_type_before_any_library_call():
    e = Engine.__new__(Engine)  # no device, no library handle: the refusal must come first
    e.n, e.p = 4, 3
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        e.vcov_robust(np.zeros(3), type="HC4")
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        e.vcov_robust(np.zeros(3), type="const")
    e._h = None
    obj = GLMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 1.0, 1.0, 1.0, 2.5, 1.0, 0.0, "gaussian", "identity",
                   0.0, 1, 2.0, 1)
    fr = Frame({"a": np.ones(3)})
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        GLM.vcov(obj, fr, fr, type="HC4")
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        GLM.coeftest(obj, fr, fr, type="const")
    lm = LMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 0.5, 2.0, 3.0, 1)
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        LM.vcov(lm, fr, fr, type="robust")
    with pytest.raises(L.IllegalArgumentException, match="type must be one of"):
        LM.coeftest(lm, fr, fr, type="HC5")


def test_signatures_and_defaults():
    sig = inspect.signature(GLM.vcov).parameters
    assert list(sig) == ["obj", "y", "x", "offset", "m", "prior", "device", "type"]
    assert sig["type"].default == "const"
    sig = inspect.signature(LM.vcov).parameters
    assert list(sig) == ["obj", "x", "y", "device", "type"] and sig["type"].default == "const"
    assert inspect.signature(GLM.coeftest).parameters["type"].default == "HC3"
    assert inspect.signature(LM.coeftest).parameters["type"].default == "HC3"
    sig = inspect.signature(Engine.vcov_robust).parameters
    assert list(sig) == ["self", "beta", "family", "link", "type", "return_meat"]
    assert sig["type"].default == "HC3" and sig["return_meat"].default is False
    assert callable(Engine.sandwich_ms)


class FakeEngine:
    """Stands in for the device: records what the API asks for and returns fixed matrices."""
    V = np.array([[4.0, 0.5], [0.5, 0.25]])
    C0 = np.array([[2.0, 0.1], [0.1, 1.0]])

    def __init__(self):
        self.calls = []

    def set_data(self, *a, **k):
        self.calls.append(("set_data", a[0].shape))

    def vcov(self, beta, fam, lnk):
        self.calls.append(("vcov", fam, lnk))
        return self.C0

    def vcov_robust(self, beta, fam, lnk, type="HC3", return_meat=False):
        self.calls.append(("vcov_robust", fam, lnk, type))
        return self.V


def test_coeftest_tables_and_vcov_routing(monkeypatch):
    from scipy import stats
    from sparkglm_amd import glm as G
    from sparkglm_amd import lm as M
    fake = FakeEngine()
    monkeypatch.setattr(G, "_engine", lambda device=0: fake)
    monkeypatch.setattr(M, "_engine", lambda device=0: fake)
    xf = Frame({"a": np.arange(6.0), "b": np.ones(6)})
    yf = Frame({"y": np.array([0.0, 1.0, 0.0, 1.0, 1.0, 0.0])})
    coefs = np.array([[1.5], [-0.2]])
    obj = GLMModel(["a", "b"], "y", coefs, [0.1, 0.2], 8.0, 9.0, 1.0, 2.0, 1.3, 1.0, -1.0, "binomial", "logit", 3.0, 2,
                   6.0, 1)
    t = GLM.coeftest(obj, yf, xf)
    assert t.columns == ["name", "estimate", "se", "stat", "pvalue"]
    assert list(t["name"]) == ["a", "b"]
    se = np.array([2.0, 0.5])
    assert np.array_equal(t["estimate"], coefs.reshape(-1)) and np.array_equal(t["se"], se)
    assert np.array_equal(t["stat"], coefs.reshape(-1) / se)
    assert np.allclose(t["pvalue"], 2.0 * stats.norm.sf(np.abs(coefs.reshape(-1) / se)), rtol=0, atol=1e-12)
    assert fake.calls[-1] == ("vcov_robust", "binomial", "logit", "HC3")
    GLM.coeftest(obj, yf, xf, type="HC1")
    assert fake.calls[-1] == ("vcov_robust", "binomial", "logit", "HC1")
    # GLM.vcov: "const" is today's call, an HC type the sandwich
    assert GLM.vcov(obj, yf, xf) is fake.C0 and fake.calls[-1] == ("vcov", "binomial", "logit")
    assert GLM.vcov(obj, yf, xf, type="HC2") is fake.V and fake.calls[-1][-1] == "HC2"

    lm = LMModel(["a", "b"], "y", coefs, [0.1, 0.2], 0.5, 0.9, 2.0, 6.0, 1)
    assert np.array_equal(LM.vcov(lm, xf, yf), 0.25 * fake.C0)  # sigma^2 inv(X'X)
    assert fake.calls[-1] == ("vcov", "gaussian", "identity")
    assert LM.vcov(lm, xf, yf, type="HC0") is fake.V
    assert fake.calls[-1] == ("vcov_robust", "gaussian", "identity", "HC0")
    t = LM.coeftest(lm, xf, yf)
    assert t.columns == ["name", "estimate", "se", "stat", "pvalue"]
    assert np.array_equal(t["se"], se) and np.array_equal(t["stat"], coefs.reshape(-1) / se)
    assert np.allclose(t["pvalue"], 2.0 * stats.t.sf(np.abs(coefs.reshape(-1) / se), 6 - 2), rtol=0, atol=1e-12)
    assert fake.calls[-1] == ("vcov_robust", "gaussian", "identity", "HC3")
