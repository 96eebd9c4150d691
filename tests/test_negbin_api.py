"""Argument checks of the negative binomial calls through ctypes and Python (no GPU).

Every check here fails before a device is touched.  "negbin without theta on the handle" needs a handle, so it
is asserted where one exists: tests/test_gpu_negbin.py::test_fixed_theta_fit_on_every_pass_path."""
import ctypes as C

import numpy as np
import pytest

import negbin_reference as NB
from sparkglm_amd import _lib as L
from sparkglm_amd import distributed as D
from sparkglm_amd.engine import Engine, glm_opts


def _pre(p):
    coefs, se = np.zeros(p), np.zeros(p)
    return L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, None, 0), (coefs, se)


@pytest.mark.parametrize("theta", [0.0, -1.0, float("nan"), float("inf")])
def test_theta_must_be_positive_and_finite(theta):
    lib = L.load()
    assert lib.sglm_set_theta(None, theta) == L.SGLM_EINVAL
    assert "theta > 0" in L.last_error()
    o, beta, out = glm_opts("negbin", "log"), np.zeros(3), np.zeros(5)
    assert lib.sglm_nb_theta_terms(None, C.byref(o), L.ptr(beta), theta, L.ptr(out)) == L.SGLM_EINVAL
    assert "theta > 0" in L.last_error()


def test_a_null_handle_is_refused():
    lib = L.load()
    assert lib.sglm_set_theta(None, 2.0) == L.SGLM_EINVAL and "handle" in L.last_error()
    t = C.c_double()
    assert lib.sglm_get_theta(None, C.byref(t)) == L.SGLM_EINVAL


@pytest.mark.parametrize("lnk", ["logit", "inverse", "probit", "cloglog"])
def test_other_links_are_refused(lnk):
    lib = L.load()
    with pytest.raises(L.IllegalArgumentException):
        L.pass_kernel_for(6001, 70, "negbin", lnk)
    o, beta, out = glm_opts("negbin", lnk), np.zeros(3), np.zeros(5)
    assert lib.sglm_nb_theta_terms(None, C.byref(o), L.ptr(beta), 2.0, L.ptr(out)) == L.SGLM_EINVAL
    assert "log, sqrt and identity" in L.last_error()
    th = C.c_double()
    assert lib.sglm_theta_ml(None, C.byref(o), L.ptr(beta), 0, 0.0, C.byref(th), None, None, None) == L.SGLM_EINVAL
    pre, keep = _pre(3)
    res = L.NbResult()
    assert lib.sglm_fit_glm_nb(None, C.byref(o), None, C.byref(pre), C.byref(res)) == L.SGLM_EINVAL
    assert "log, sqrt and identity" in L.last_error()
    assert lib.sglm_fit_glm_start(None, C.byref(o), L.ptr(beta), C.byref(pre)) == L.SGLM_EINVAL
    assert "family/link" in L.last_error()


def test_fit_glm_start_checks_its_arguments():
    lib = L.load()
    o = glm_opts("poisson", "log")
    pre, keep = _pre(3)
    assert lib.sglm_fit_glm_start(None, C.byref(o), None, C.byref(pre)) == L.SGLM_EINVAL
    assert "beta_start" in L.last_error()
    assert lib.sglm_fit_glm_start(None, C.byref(o), L.ptr(np.zeros(3)), None) == L.SGLM_EINVAL
    # the Python mirror refuses a start of the wrong length before it calls the library
    e = object.__new__(Engine)
    e.p, e._h, e._lib = 4, None, lib
    with pytest.raises(L.IllegalArgumentException, match="Dimension mismatch"):
        e.fit_glm("poisson", "log", start=np.zeros(5))
    with pytest.raises(L.IllegalArgumentException, match="Dimension mismatch"):
        e.theta_ml(np.zeros(3))


def test_the_external_backend_refuses_negbin():
    part = lambda *a: np.zeros(2 * 3 // 2 + 2 + L.NS)
    with pytest.raises(L.IllegalArgumentException, match="external backend"):
        D.fit_glm_external(2, lambda: (1.0, 2.0), part, family="negbin", link="log")


@pytest.mark.parametrize("n,p,fs,kind,stem", [
    (3001, 20, 1, "narrow", "irls_narrow_kernel<2,"), (6001, 64, 1, "narrow", "irls_narrow_kernel<4,"),
    (6001, 70, 1, "fused", "irls_pass_kernel<5,"), (6001, 150, 1, "fused-split", "irls_pass_r_kernel<10,"),
    (6001, 70, 5, "fused-split", "irls_pass_r_kernel<5,")])
def test_pass_kernel_names(n, p, fs, kind, stem):
    for lnk, slot in (("log", "log"), ("sqrt", "runtime"), ("identity", "runtime")):
        k, name = L.pass_kernel_for(n, p, "negbin", lnk, fused_split=fs)
        assert k == kind and name == f"{stem}negbin,{slot}>", (k, name)
    assert L.pass_kernel_for(5001, 290, "negbin", "log") == ("wide", "wide_gram_kernel<resident>")
    assert L.pass_kernel_for(6000, 520, "negbin", "log", procedural=True)[0] == "wide-procedural"


def test_structs_and_tables():
    assert L.FAMILIES["negbin"] == 4 and L.NEGBIN_LINKS == NB.LINKS
    assert C.sizeof(L.NbOpts) == 32 and C.sizeof(L.NbResult) == 40   # the C layout of sglm_nb_opts / sglm_nb_result
    o = glm_opts("negbin", "sqrt")
    assert (o.family, o.link) == (4, 6)


def test_glm_fit_string_dispatch_is_unchanged():
    from sparkglm_amd import glm as G
    assert G._engine_family_link("negbin", "log") == ("binomial", "cloglog")  # unknown family: binomial, as before
    m = G.GLMModel(["a"], "y", np.zeros((1, 1)), [1.0], 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0, "negbin", "log", 4.0, 1,
                   3.0, 1, theta=2.0)
    assert G._model_family_link(m) == ("negbin", "log") and G._dispersion(m) == 1.0
    m.link = "inverse"
    with pytest.raises(L.IllegalArgumentException):
        G._model_family_link(m)


def test_the_overlapped_wide_row_kernel_keeps_the_budget():
    """tests/test_residency.py's budget for the negative binomial's overlapped row kernels (the inline log rows
    and the run-time-link rows): at most 96 VGPRs and no scratch, so that one such workgroup fits a SIMD beside
    the two persistent Gram workgroups."""
    from test_residency import _alloc, _kernel_meta
    rows = {k: v for k, v in _kernel_meta().items() if "wide_rows_nb_ov_kernel" in k}
    assert len(rows) == 2  # <negbin, log> and <negbin, runtime>
    for v in rows.values():
        assert v["private_segment_fixed_size"] == 0 and _alloc(v["vgpr_count"]) <= 96


def test_polygamma_is_bounded_and_matches_scipy(tmp_path):
    """csrc/polygamma.hpp compiled for the host: digamma_pos / trigamma_pos against scipy on (0, 1e6], and NaN --
    returned at once, the recurrence never entered -- for every argument outside the domain: zero, negatives up
    to the magnitudes at which x + 1 == x (a loop on `x < 10` alone would never end there), -Inf, NaN."""
    import os
    import shutil
    import subprocess
    from scipy.special import digamma, polygamma
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "pg.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "polygamma.hpp"\n'
                   'int main(int argc, char** argv) {\n'
                   '  for (int i = 1; i < argc; ++i) {\n'
                   '    const double x = std::strtod(argv[i], nullptr);\n'
                   '    std::printf("%.17g %.17g\\n", sglm::digamma_pos(x), sglm::trigamma_pos(x));\n'
                   '  }\n  return 0;\n}\n')
    exe = tmp_path / "pg"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(root, "sparkglm_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    good = [1e-150, 1e-8, 0.01, 0.5, 0.7, 1.0, 2.5, 5.999, 6.0, 9.999, 10.0, 30.0, 170.01, 1e4, 100000.01, 1e6]
    bad = ["0", "-0.5", "-3", "-1e9", "-1e12", "-9.1e15", "-1e30", "-1e300", "-inf", "nan"]
    out = subprocess.run([str(exe)] + [repr(v) for v in good] + bad, check=True, capture_output=True, text=True,
                         timeout=20).stdout.split("\n")
    got = np.array([[float(t) for t in ln.split()] for ln in out if ln.strip()])
    assert got.shape == (len(good) + len(bad), 2)
    g = np.array(good)
    e1 = np.abs(got[: len(good), 0] - digamma(g)) / np.maximum(np.abs(digamma(g)), 1.0)
    e2 = np.abs(got[: len(good), 1] - polygamma(1, g)) / polygamma(1, g)
    print(f"\npolygamma: digamma max err {e1.max():.1e}, trigamma max rel err {e2.max():.1e}")
    assert e1.max() < 1e-14 and e2.max() < 1e-14
    assert np.all(np.isnan(got[len(good):]))


def test_summary_of_a_negbin_model_prints_theta_and_its_aic():
    from sparkglm_amd import glm as G
    m = G.GLMModel(["a", "b"], "y", np.array([[0.5], [-1.25]]), [0.1, 0.2], 98.0, 99.0, 110.0, 150.0, 1.1, 108.0,
                   -123.456, "negbin", "log", 252.912, 4, 100.0, 1, theta=2.3456789, theta_se=0.1234567,
                   twologlik=-246.912)
    text = G.GLM.summary_string(m)
    lines = text.split("\n")
    k = lines.index("AIC: 252.91")   # obj.aic = -2 loglik + 2 (p + 1), five significant digits
    assert lines[k + 1: k + 4] == ["Theta: 2.34568", "Std. Err.: 0.123457", "2 x log-likelihood: -246.912"]
    assert text.count("AIC: ") == 1 and "Number of Fisher Scoring iterations: 4" in text
    m.theta_se = m.twologlik = None   # theta given, not estimated: no standard error, createObj's AIC
    m.aic = 250.912
    lines = G.GLM.summary_string(m).split("\n")
    k = lines.index("AIC: 250.91")
    assert lines[k + 1] == "Theta: 2.34568" and not any(ln.startswith("Std. Err.") for ln in lines)
    with pytest.raises(RuntimeError):
        G._nb_summary("no such line\n", m, L.load())
