"""The Firth entry points without a device: the ctypes mirrors of sglm_firth_opts / sglm_firth_info, the exports,
the refusals that precede any launch (reached with a null handle) and GLM.fit_firth's argument checks."""
import ctypes as C

import numpy as np
import pytest

from sparkglm_amd import _lib as L
from sparkglm_amd.frame import Frame
from sparkglm_amd.glm import GLM

FIRTH_PAIRS = [(0, 0), (0, 1), (0, 2), (2, 4), (2, 3), (2, 6)]  # (family, link) of include/sglm.h


def test_struct_layouts_and_exports():
    assert C.sizeof(L.FirthOpts) == 16
    assert [L.FirthOpts.epsilon.offset, L.FirthOpts.maxit.offset, L.FirthOpts.max_halvings.offset] == [0, 8, 12]
    assert C.sizeof(L.FirthInfo) == 72
    I = L.FirthInfo
    assert [I.iterations.offset, I.converged.offset, I.halvings.offset, I.deviance.offset, I.pen_deviance.offset,
            I.logdet.offset, I.score_inf.offset, I.sum_hat.offset, I.firth_ms.offset, I.pass_ms.offset] == \
        [0, 4, 8, 16, 24, 32, 40, 48, 56, 64]
    for name in ("sglm_fit_glm_firth", "sglm_firth_pass", "sglm_get_firth_ms"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.load().sglm_abi_version() == 8
    assert L.FIRTH_LINKS == {"binomial": ("logit", "probit", "cloglog"), "poisson": ("log", "identity", "sqrt")}


def _calls(lib):
    coefs, se = np.zeros(3), np.zeros(3)
    pre = L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, None, 0)
    keep = (coefs, se, pre)
    fit = lambda op, fo=None: lib.sglm_fit_glm_firth(None, C.byref(op), None if fo is None else C.byref(fo), None,
                                                     C.byref(pre), None)
    step = lambda op: lib.sglm_firth_pass(None, C.byref(op), L.ptr(coefs), None, None, None, None)
    return fit, step, keep


def test_refusals_before_any_device_call():
    """The checks that need no handle come first: a null handle is reached only after them."""
    lib = L.load()
    fit, step, keep = _calls(lib)
    opts = lambda f, l: L.GlmOpts(f, l, 1e-6, 0, 0, 0, 0)
    for f, l in FIRTH_PAIRS:
        for call in (fit, step):
            assert call(opts(f, l)) == L.SGLM_EINVAL and "null engine handle" in L.last_error(), (f, l)
    # gaussian, gamma, negbin (a dispersion), and pairs that are no pairs at all
    for f, l in ((1, 3), (1, 4), (3, 5), (3, 4), (4, 4), (4, 6), (0, 4), (2, 0), (7, 0)):
        for call in (fit, step):
            assert call(opts(f, l)) == L.SGLM_EINVAL and "Firth fit takes binomial" in L.last_error(), (f, l)
    for eps in (0.0, -1e-8, float("nan"), float("inf")):
        assert fit(opts(0, 0), L.FirthOpts(eps, 100, 12)) == L.SGLM_EINVAL and "epsilon" in L.last_error(), eps
    assert fit(opts(0, 0), L.FirthOpts(1e-8, -1, 12)) == L.SGLM_EINVAL and "maxit" in L.last_error()
    assert fit(opts(0, 0), L.FirthOpts(1e-8, 100, 12)) == L.SGLM_EINVAL and "null engine handle" in L.last_error()
    o = opts(0, 0)
    assert lib.sglm_fit_glm_firth(None, C.byref(o), None, None, None, None) == L.SGLM_EINVAL and "out" in L.last_error()
    assert lib.sglm_firth_pass(None, C.byref(o), None, None, None, None, None) == L.SGLM_EINVAL
    assert "beta" in L.last_error()
    assert lib.sglm_fit_glm_firth(None, None, None, None, None, None) == L.SGLM_EINVAL
    assert lib.sglm_get_firth_ms(None, None) == L.SGLM_EINVAL


def test_fit_firth_argument_checks():
    """Refused in Python, before an engine is made."""
    y = Frame({"y": np.array([0.0, 1.0, 1.0, 0.0])})
    x = Frame({"(Intercept)": np.ones(4), "x": np.array([0.1, 0.4, 0.2, 0.9])})
    for fam in ("gaussian", "gamma", "negbin", "tweedie"):
        with pytest.raises(L.IllegalArgumentException, match="binomial or poisson"):
            GLM.fit_firth(y, x, fam, "log")
    for fam, lnk in (("binomial", "log"), ("poisson", "logit"), ("poisson", "inverse")):
        with pytest.raises(L.IllegalArgumentException, match="supports only"):
            GLM.fit_firth(y, x, fam, lnk)
    for eps in (0.0, -1.0, float("nan"), float("inf"), "1e-8"):
        with pytest.raises(L.IllegalArgumentException, match="epsilon"):
            GLM.fit_firth(y, x, epsilon=eps)
    for maxit in (-1, 2.5):
        with pytest.raises(L.IllegalArgumentException, match="maxit"):
            GLM.fit_firth(y, x, maxit=maxit)
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        GLM.fit_firth(y, x, prior=Frame({"w": np.ones(3)}))
