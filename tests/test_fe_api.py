"""The fixed-effects entry points without a GPU: the symbols are exported, the argument checks that touch no
device refuse, and the model layer's array logic (coding of labels, intercept removal, dropping of
uninformative groups) runs on Frames."""
import ctypes as C

import numpy as np
import pytest

from sparkglm_amd import _lib as L
from sparkglm_amd.frame import Frame
from sparkglm_amd.glm import GLM, GLMModel, fe_offsets

NEW = ("sglm_fit_glm_fe", "sglm_fe_pass", "sglm_vcov_fe", "sglm_get_fe_ms")


def test_symbols_are_exported_and_listed():
    lib = L.load()
    for s in NEW:
        assert hasattr(lib, s) and s in L.EXPORTS
    assert C.sizeof(L.FeInfo) == 48  # int32 + padding, five doubles: sglm_fe_info


def test_refusals_that_touch_no_device():
    lib = L.load()
    o = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0)  # poisson / log
    bad = L.GlmOpts(2, 0, 1e-6, 0, 0, 0, 0)  # poisson / logit
    p = 3
    coefs, se, alpha, cov = np.zeros(p), np.zeros(p), np.zeros(4), np.zeros((p, p), order="F")
    pre = L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, None, 0)
    info = L.FeInfo()
    E = L.SGLM_EINVAL
    assert lib.sglm_fit_glm_fe(None, C.byref(o), C.byref(pre), L.ptr(alpha), C.byref(info)) == E  # null handle
    assert "null engine handle" in L.last_error()
    assert lib.sglm_fit_glm_fe(None, C.byref(o), None, L.ptr(alpha), None) == E
    assert lib.sglm_fit_glm_fe(None, C.byref(o), C.byref(pre), None, None) == E
    assert "alpha" in L.last_error()
    assert lib.sglm_fit_glm_fe(None, C.byref(bad), C.byref(pre), L.ptr(alpha), None) == E
    assert "family/link" in L.last_error()
    assert lib.sglm_fit_glm_fe(None, None, C.byref(pre), L.ptr(alpha), None) == E
    assert lib.sglm_fe_pass(None, C.byref(o), None, None, None, None, None, None) == E
    assert lib.sglm_fe_pass(None, None, None, None, None, None, None, None) == E
    assert lib.sglm_vcov_fe(None, C.byref(o), L.ptr(coefs), L.ptr(alpha), 1, 1, 1, cov.ctypes.data_as(L.dp), None) == E
    assert lib.sglm_vcov_fe(None, C.byref(o), None, L.ptr(alpha), 0, 0, 0, cov.ctypes.data_as(L.dp), None) == E
    for hc in (2, 3):  # HC2 / HC3 under clustering, before the handle is looked at
        assert lib.sglm_vcov_fe(None, C.byref(o), L.ptr(coefs), L.ptr(alpha), 1, hc, 1, cov.ctypes.data_as(L.dp),
                                None) == E
        assert "HC2 / HC3" in L.last_error()
    t = C.c_double()
    assert lib.sglm_get_fe_ms(None, C.byref(t), C.byref(t), C.byref(t), C.byref(t)) == E


def frames(n=60, seed=0):
    rng = np.random.default_rng(seed)
    firm = np.array([f"firm{(i // 6) % 5}" for i in range(n)])
    x = Frame({"(Intercept)": np.ones(n), "a": rng.normal(size=n), "b": rng.normal(size=n)})
    y = rng.poisson(2.0, n).astype(np.float64)
    return x, y, firm


def test_fe_data_codes_labels_drops_the_intercept_and_uninformative_groups(capsys):
    x, y, firm = frames()
    y[firm == "firm3"] = 0.0
    prior = np.ones(len(y))
    out = GLM._fe_data(Frame({"y": y}), x, Frame({"firm": firm}), "poisson", "log", None, None,
                       Frame({"w": prior}), True)
    labels, codes, ngroups, nrows = out.labels, out.codes, out.dropped, out.dropped_rows
    assert (out.fam, out.lnk) == ("poisson", "log") and out.names == ["a", "b"] and out.X.shape == (48, 2)
    assert list(labels) == ["firm0", "firm1", "firm2", "firm4"] and ngroups == 1 and nrows == 12
    assert codes.min() == 0 and codes.max() == 3 and len(codes) == 48 and len(out.y) == 48 and len(out.prior) == 48
    assert np.array_equal(labels[codes], firm[firm != "firm3"])
    assert "1 fixed effect(s) (12 rows) removed" in capsys.readouterr().out
    # kept when asked: the engine then refuses the fit
    out = GLM._fe_data(Frame({"y": y}), x, Frame({"firm": firm}), "poisson", "log", None, None, None, False)
    assert out.X.shape == (60, 2) and len(out.labels) == 5 and out.dropped == 0
    # integer labels, gaussian: nothing is uninformative
    out = GLM._fe_data(Frame({"y": y}), x, Frame({"id": np.arange(60) % 4 + 10}), "gaussian", "identity", None, None,
                       None, True)
    assert list(out.labels) == [10, 11, 12, 13] and out.dropped == 0


def test_model_layer_refusals_without_a_device():
    x, y, firm = frames()
    yf, ff = Frame({"y": y}), Frame({"firm": firm})
    with pytest.raises(L.IllegalArgumentException, match="only one column"):
        GLM.fit_fe(yf, x, Frame({"f": firm, "g": firm}))
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        GLM.fit_fe(yf, x, Frame({"f": firm[:-1]}))
    with pytest.raises(L.IllegalArgumentException, match="beside the intercept"):
        GLM.fit_fe(yf, Frame({"one": np.ones(len(y))}), ff)
    with pytest.raises(L.IllegalArgumentException, match="links"):
        GLM.fit_fe(yf, x, ff, "negbin", "logit", theta=1.0)
    plain = GLMModel(["a"], "y", np.zeros((1, 1)), [0.0], 1, 1, 0, 0, 1, 0, 0, "poisson", "log", 0, 0, 2, 1)
    with pytest.raises(L.IllegalArgumentException, match="GLM.fit_fe model"):
        plain.predict(Frame({"a": np.zeros(2)}), fe=Frame({"f": np.array(["u", "v"])}))
    fe_model = GLMModel(["a"], "y", np.zeros((1, 1)), [0.0], 1, 1, 0, 0, 1, 0, 0, "poisson", "log", 0, 0, 2, 1,
                        fixef={"u": 0.5})
    with pytest.raises(L.IllegalArgumentException, match="predicts with fe"):
        fe_model.predict(Frame({"a": np.zeros(2)}))
    assert np.isnan(fe_offsets(fe_model.fixef, np.array(["u", "v"]))[1])
