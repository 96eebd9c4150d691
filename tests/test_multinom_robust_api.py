"""sglm_vcov_multinom_robust without a device: the export, its argument types, the refusals before any launch."""
import ctypes as C

import numpy as np

from sparkglm_amd import _lib as L


def test_export_and_argtypes():
    lib = L.load()
    for name in ("sglm_vcov_multinom_robust", "sglm_set_multinom_route"):
        assert name in L.EXPORTS and hasattr(lib, name)
    dp, h = L.dp, lib.sglm_multinom_pass.argtypes[0]
    assert lib.sglm_vcov_multinom_robust.argtypes == [h, C.c_int, dp, C.c_int, dp, dp]
    assert lib.sglm_set_multinom_route.argtypes == [h, C.c_int]


def test_refusals_before_any_device_call():
    lib = L.load()
    B, cov = np.zeros(64), np.zeros(64 * 64)
    call = lambda K, hc, b=B, c=cov: lib.sglm_vcov_multinom_robust(None, K, L.ptr(b), hc, L.ptr(c), None)
    for K, b, c, msg in ((-1, B, cov, "n_classes <= 16"), (1, B, cov, "n_classes <= 16"), (17, B, cov, "n_classes <= 16"),
                         (3, None, cov, "B, cov"), (3, B, None, "B, cov")):
        assert call(K, 0, b, c) == L.SGLM_EINVAL and msg in L.last_error(), (K, msg)
    for hc in (2, 3, -1, 4, 0, 1):
        assert call(3, hc) == L.SGLM_EINVAL and ("null engine" if hc in (0, 1) else "HC0 or SGLM_HC1") in L.last_error(), hc
    assert lib.sglm_set_multinom_route(None, 1) == L.SGLM_EINVAL and "null engine handle" in L.last_error()
