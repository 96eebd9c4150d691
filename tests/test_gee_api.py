"""The GEE entry points without a device: the refusals that precede any launch, the ctypes mirrors of
sglm_gee_opts / sglm_gee_info, and the Python factorisation of cluster labels."""
import ctypes as C

import numpy as np
import pytest

import fe_reference as FR
import gee_reference as GR
from sparkglm_amd import _lib as L
from sparkglm_amd.engine import _codes, gee_opts


def test_struct_layouts():
    assert C.sizeof(L.GeeOpts) == 16 and L.GeeOpts.rho.offset == 8 and L.GeeOpts.fix_rho.offset == 4
    assert C.sizeof(L.GeeInfo) == 64
    assert [L.GeeInfo.rho.offset, L.GeeInfo.phi.offset, L.GeeInfo.N.offset, L.GeeInfo.G_eff.offset,
            L.GeeInfo.n_max.offset, L.GeeInfo.rows_ms.offset, L.GeeInfo.gram_ms.offset] == [0, 8, 16, 24, 28, 32, 56]
    assert L.CORSTRS == {"independence": 0, "exchangeable": 1}
    for name in ("sglm_fit_glm_gee", "sglm_gee_pass", "sglm_vcov_gee", "sglm_get_gee_ms"):
        assert name in L.EXPORTS and hasattr(L.load(), name)


def test_gee_opts():
    g = gee_opts()
    assert (g.corstr, g.fix_rho, g.rho) == (1, 0, 0.0)
    g = gee_opts("exchangeable", -0.01)
    assert (g.corstr, g.fix_rho, g.rho) == (1, 1, -0.01)
    assert gee_opts("independence").corstr == 0
    with pytest.raises(L.IllegalArgumentException, match="corstr"):
        gee_opts("ar1")
    for bad in (1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(L.IllegalArgumentException, match="below 1"):
            gee_opts("exchangeable", bad)


def test_refusals_before_any_device_call():
    """The checks that need no handle come first: a null handle is reached only after them."""
    lib = L.load()
    o = L.GlmOpts(2, 4, 1e-6, 0, 0, 0, 0)
    coefs, se = np.zeros(3), np.zeros(3)
    pre = L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, None, 0)
    cov = np.zeros(9)
    calls = dict(
        fit=lambda g, op=o: lib.sglm_fit_glm_gee(None, C.byref(op), C.byref(g), C.byref(pre), None),
        step=lambda g, op=o: lib.sglm_gee_pass(None, C.byref(op), C.byref(g), None, None, None, None, None, None, None),
        cov=lambda g, op=o: lib.sglm_vcov_gee(None, C.byref(op), C.byref(g), L.ptr(coefs), 0.2, 1, 0, L.ptr(cov), None))
    for name, call in calls.items():
        assert call(L.GeeOpts(7, 0, 0.0)) == L.SGLM_EINVAL and "corstr" in L.last_error(), name
        assert call(L.GeeOpts(1, 0, 0.0)) == L.SGLM_EINVAL and "null engine handle" in L.last_error(), name
        assert call(L.GeeOpts(1, 0, 0.0), L.GlmOpts(2, 0, 1e-6, 0, 0, 0, 0)) == L.SGLM_EINVAL  # poisson / logit
        assert "family/link" in L.last_error(), name
    for name in ("fit", "step"):
        assert calls[name](L.GeeOpts(1, 1, 1.0)) == L.SGLM_EINVAL and "below 1" in L.last_error(), name
        assert calls[name](L.GeeOpts(0, 1, 1.0)) == L.SGLM_EINVAL and "null engine" in L.last_error(), name  # rho unused
    assert lib.sglm_vcov_gee(None, C.byref(o), C.byref(L.GeeOpts(1, 0, 0.0)), L.ptr(coefs), 1.0, 1, 0, L.ptr(cov),
                             None) == L.SGLM_EINVAL and "below 1" in L.last_error()
    assert lib.sglm_fit_glm_gee(None, C.byref(o), None, None, None) == L.SGLM_EINVAL and "out" in L.last_error()
    assert lib.sglm_vcov_gee(None, C.byref(o), None, None, 0.2, 1, 0, None, None) == L.SGLM_EINVAL
    assert lib.sglm_get_gee_ms(None, None) == L.SGLM_EINVAL


def test_labels_of_any_dtype_factorise_to_dense_codes():
    ids, G = FR.make_ids("two_level", 200, 128)
    for labels in (ids * 10 + 3, np.array([f"g{k:02d}" for k in ids]), ids.astype(np.float64)):
        codes, n = _codes(labels, None, "G", "cluster id")
        assert n == G and codes.dtype == np.int32 and np.array_equal(codes, ids)
    assert L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0] == 128  # the tile the CPU reference tests assume
    # the reference's counts: rows of positive prior weight only
    c = GR.make_case("poisson", "log", 200, 3, ids, G, 1)
    pw = c["pw"].copy()
    pw[ids == 2] = 0.0
    r = GR.rows(c["X"], c["y"], c["beta"], "poisson", "log", off=c["off"], pw=pw)
    gs = GR.group_sums(c["X"], r, ids, G)
    assert gs["n"][2] == 0.0 and gs["n"].sum() == np.sum(pw > 0) and not gs["s"][2].any() and gs["Q"][2] == 0.0
