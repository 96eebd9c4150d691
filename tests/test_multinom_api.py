"""The multinomial entry points without a device: the ctypes mirrors of sglm_multinom_opts / sglm_multinom_info,
the exports, the refusals that precede any launch (reached with a null handle), and Multinom's level coding and
argument checks.  (n_classes - 1) * p <= 1024 needs p, which only a handle knows: without a device it is checked
through Multinom.fit, which refuses before an engine is made; tests/test_gpu_multinom.py checks the C ABI's.)"""
import ctypes as C

import numpy as np
import pytest

from sparkglm_amd import Multinom, _lib as L
from sparkglm_amd.frame import Frame
from sparkglm_amd.multinom import code_levels, softmax_link


def test_struct_layouts_and_exports():
    O, I = L.MultinomOpts, L.MultinomInfo
    assert C.sizeof(O) == 24
    assert [O.n_classes.offset, O.epsilon.offset, O.max_iter.offset, O.max_halvings.offset] == [0, 8, 16, 20]
    assert C.sizeof(I) == 16 + 5 * 8 + 16 * 8
    assert [I.iter.offset, I.halvings.offset, I.converged.offset, I.deviance.offset, I.null_deviance.offset,
            I.loglik.offset, I.aic.offset, I.score_inf.offset, I.class_weight.offset] == \
        [0, 4, 8, 16, 24, 32, 40, 48, 56]
    lib = L.load()
    for name in ("sglm_fit_multinom", "sglm_multinom_pass", "sglm_get_multinom_ms"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.sglm_abi_version() == 8
    dp, h = L.dp, lib.sglm_multinom_pass.argtypes[0]
    assert lib.sglm_multinom_pass.argtypes == [h, C.c_int, dp, dp, dp, dp, dp]
    assert lib.sglm_fit_multinom.argtypes == [h, C.POINTER(O), dp, dp, dp, dp, C.POINTER(I)]
    assert lib.sglm_get_multinom_ms.argtypes == [h, dp, dp, dp, dp]
    assert (L.MULTINOM_MAX_K, L.MULTINOM_MAX_Q) == (16, 1024)


def test_refusals_before_any_device_call():
    """The checks that need no handle come first: a null handle is reached only after them."""
    lib = L.load()
    B = np.zeros(64)
    step = lambda K, b=B: lib.sglm_multinom_pass(None, K, L.ptr(b), None, None, None, None)
    fit = lambda o, b=B: lib.sglm_fit_multinom(None, None if o is None else C.byref(o), None, L.ptr(b), None, None, None)
    for K in (-1, 0, 1, 17, 100):
        assert step(K) == L.SGLM_EINVAL and "n_classes <= 16" in L.last_error(), K
        assert fit(L.MultinomOpts(K, 1e-8, 100, 12)) == L.SGLM_EINVAL and "n_classes <= 16" in L.last_error(), K
    for K in (2, 3, 16):
        assert step(K) == L.SGLM_EINVAL and "null engine handle" in L.last_error(), K
        assert fit(L.MultinomOpts(K, 1e-8, 100, 12)) == L.SGLM_EINVAL and "null engine handle" in L.last_error(), K
    assert step(3, None) == L.SGLM_EINVAL and "requirement failed: B" in L.last_error()
    assert fit(L.MultinomOpts(3, 1e-8, 100, 12), None) == L.SGLM_EINVAL and "requirement failed: B" in L.last_error()
    assert fit(None) == L.SGLM_EINVAL and "opts" in L.last_error()
    for eps in (0.0, -1e-8, float("nan"), float("inf")):
        assert fit(L.MultinomOpts(3, eps, 100, 12)) == L.SGLM_EINVAL and "epsilon" in L.last_error(), eps
    assert fit(L.MultinomOpts(3, 1e-8, -1, 12)) == L.SGLM_EINVAL and "max_iter" in L.last_error()
    assert fit(L.MultinomOpts(3, 1e-8, 100, -1)) == L.SGLM_EINVAL and "max_halvings" in L.last_error()
    t = C.c_double()
    assert lib.sglm_get_multinom_ms(None, C.byref(t), C.byref(t), C.byref(t), C.byref(t)) == L.SGLM_EINVAL


def test_level_coding():
    lev, codes = code_levels(np.array(["setosa", "virginica", "setosa", "versicolor"]))
    assert list(lev) == ["setosa", "versicolor", "virginica"] and codes.dtype == np.float64
    assert list(codes) == [0.0, 2.0, 0.0, 1.0]
    lev, codes = code_levels(np.array([10, 3, 3, 7]))
    assert list(lev) == [3, 7, 10] and list(codes) == [2.0, 0.0, 0.0, 1.0]
    lev, codes = code_levels(np.array([True, False]))
    assert list(codes) == [1.0, 0.0]
    pr = softmax_link(np.array([[0.0, 0.0], [800.0, -800.0], [-800.0, -900.0]]))
    assert np.allclose(pr[0], 1 / 3) and np.all(np.isfinite(pr)) and np.allclose(pr.sum(axis=1), 1.0)
    assert pr[1, 1] == 1.0 and pr[2, 0] == 1.0


def test_fit_argument_checks():
    """Refused in Python, before an engine is made."""
    x = Frame({"(Intercept)": np.ones(4), "x": np.array([0.1, 0.4, 0.2, 0.9])})
    y = Frame({"y": np.array(["a", "b", "c", "a"])})
    with pytest.raises(L.IllegalArgumentException, match="number of classes"):
        Multinom.fit(Frame({"y": np.array(["a", "a", "a", "a"])}), x)
    big = Frame({"y": np.arange(18)})
    with pytest.raises(L.IllegalArgumentException, match="number of classes"):
        Multinom.fit(big, Frame({"(Intercept)": np.ones(18)}))
    wide = Frame({f"x{j}": np.ones(4) for j in range(600)})
    with pytest.raises(L.IllegalArgumentException, match=r"\(n_classes - 1\) \* p <= 1024 \(got 1200\)"):
        Multinom.fit(y, wide)
    for eps in (0.0, -1.0, float("nan"), float("inf"), "1e-8"):
        with pytest.raises(L.IllegalArgumentException, match="epsilon"):
            Multinom.fit(y, x, epsilon=eps)
    for k in (-1, 2.5):
        with pytest.raises(L.IllegalArgumentException, match="max_iter"):
            Multinom.fit(y, x, max_iter=k)
        with pytest.raises(L.IllegalArgumentException, match="max_halvings"):
            Multinom.fit(y, x, max_halvings=k)
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        Multinom.fit(y, x, prior=Frame({"w": np.ones(3)}))
    with pytest.raises(L.IllegalArgumentException, match="same number of rows"):
        Multinom.fit(Frame({"y": np.array(["a", "b"])}), x)
