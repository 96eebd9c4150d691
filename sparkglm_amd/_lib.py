"""ctypes binding of libsglm_hip.so (the C ABI declared in include/sglm.h).

The library is built in-tree (sparkglm_amd/lib/) by ``make -C sparkglm_amd/csrc`` or
``__graft_entry__.build()``.  There is no fallback: if the HIP library is missing the
import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SGLM_LIB selects another in-tree build of the same library (A/B kernel comparisons in tools/)
LIB_PATH = os.environ.get("SGLM_LIB") or os.path.join(HERE, "lib", "libsglm_hip.so")

SGLM_OK, SGLM_EINVAL, SGLM_ESINGULAR, SGLM_EHIP, SGLM_ECOMM, SGLM_ENOMEM = range(6)
FAMILIES = {"binomial": 0, "gaussian": 1, "poisson": 2, "gamma": 3, "negbin": 4}
LINKS = {"logit": 0, "probit": 1, "cloglog": 2, "identity": 3, "log": 4, "inverse": 5, "sqrt": 6}
CANONICAL_LINK = {"gaussian": "identity", "poisson": "log", "gamma": "inverse"}
# the links of each extension family (R's family objects; include/sglm.h enum sglm_link), canonical first
FAMILY_LINKS = {"gaussian": ("identity", "log", "inverse"), "poisson": ("log", "identity", "sqrt"),
                "gamma": ("inverse", "identity", "log")}
NEGBIN_LINKS = ("log", "sqrt", "identity")  # MASS::negative.binomial's; theta lives on the engine handle
INIT_SINGLE, INIT_MULTIPLE = 0, 1
NS = 8
S_DEV, S_PEARSON, S_LL, S_BAD, S_AUX0, S_AUX1, S_AUX2, S_SUMW = range(8)

# Symbols include/sglm.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "sglm_abi_version", "sglm_last_error", "sglm_device_count", "sglm_create", "sglm_destroy",
    "sglm_set_data", "sglm_set_data_device", "sglm_synth", "sglm_synth_procedural", "sglm_get_data", "sglm_set_comm",
    "sglm_rccl_unique_id", "sglm_set_comm_rccl", "sglm_fit_glm", "sglm_fit_lm", "sglm_irls_pass", "sglm_irls_step",
    "sglm_irls_iterations", "sglm_predict", "sglm_get_stats", "sglm_reset_stats",
    "sglm_fit_glm_external", "sglm_fit_lm_external", "sglm_glm_create_obj", "sglm_glm_summary",
    "sglm_lm_summary", "sglm_sig_digits", "sglm_round_digits", "sglm_java_double_string",
    "sglm_pval_normal", "sglm_pval_t", "sglm_create_device", "sglm_create_multi", "sglm_handle_devices", "sglm_reserve", "sglm_set_rows",
    "sglm_predict_glm", "sglm_predict_new", "sglm_local_comm_create", "sglm_local_comm_destroy",
    "sglm_local_comm_rank", "sglm_local_allreduce", "sglm_set_comm_rank", "sglm_pass_kernel_for",
    "sglm_vcov", "sglm_influence", "sglm_predict_new_se", "sglm_get_influence_ms",
    "sglm_vcov_robust", "sglm_get_sandwich_ms",
    "sglm_set_clusters", "sglm_vcov_cluster", "sglm_get_cluster_ms", "sglm_cluster_plan",
    "sglm_set_theta", "sglm_get_theta", "sglm_get_theta_ms", "sglm_nb_theta_terms", "sglm_theta_ml", "sglm_fit_glm_start",
    "sglm_fit_glm_nb",
    "sglm_fit_glm_fe", "sglm_fe_pass", "sglm_vcov_fe", "sglm_get_fe_ms",
    "sglm_set_fe2", "sglm_fe2_plan", "sglm_fit_glm_fe2", "sglm_fe2_pass", "sglm_vcov_fe2", "sglm_get_fe2_ms",
    "sglm_fit_glm_gee", "sglm_gee_pass", "sglm_vcov_gee", "sglm_get_gee_ms",
    "sglm_fit_glm_firth", "sglm_firth_pass", "sglm_get_firth_ms",
    "sglm_fit_multinom", "sglm_multinom_pass", "sglm_get_multinom_ms",
]
PREDICT_LINK, PREDICT_RESPONSE = 0, 1
RESID_TYPES = {"response": 0, "working": 1, "pearson": 2, "deviance": 3}  # enum sglm_resid_type
HC_TYPES = {"HC0": 0, "HC1": 1, "HC2": 2, "HC3": 3}  # enum sglm_hc_type

dp = C.POINTER(C.c_double)


class GlmOpts(C.Structure):
    _fields_ = [("family", C.c_int), ("link", C.c_int), ("tol", C.c_double), ("verbose", C.c_int),
                ("max_iter", C.c_int), ("init_mode", C.c_int), ("npart", C.c_int)]


class PreGLM(C.Structure):
    _fields_ = [("coefs", dp), ("std_err", dp), ("deviance", C.c_double), ("null_deviance", C.c_double),
                ("pearson", C.c_double), ("loglik", C.c_double), ("iter", C.c_int), ("nrow", C.c_double),
                ("npart", C.c_int), ("dev_trace", dp), ("max_trace", C.c_int)]


class NbOpts(C.Structure):
    _fields_ = [("maxit", C.c_int), ("epsilon", C.c_double), ("theta_limit", C.c_int), ("theta_eps", C.c_double)]


class NbResult(C.Structure):
    _fields_ = [("theta", C.c_double), ("se_theta", C.c_double), ("twologlik", C.c_double),
                ("outer_iter", C.c_int), ("theta_warn", C.c_int), ("converged", C.c_int)]


class FeInfo(C.Structure):
    _fields_ = [("G_eff", C.c_int32), ("df_residual", C.c_double), ("weights_ms", C.c_double),
                ("sum_ms", C.c_double), ("combine_ms", C.c_double), ("gram_ms", C.c_double)]


class Fe2Opts(C.Structure):
    _fields_ = [("sweep_tol", C.c_double), ("max_sweeps", C.c_int)]


class Fe2Info(C.Structure):
    _fields_ = [("G_eff", C.c_int32), ("H_eff", C.c_int32), ("ncomp", C.c_int32), ("sweeps_last", C.c_int32),
                ("sweeps_total", C.c_int64), ("df_residual", C.c_double), ("weights_ms", C.c_double),
                ("sum1_ms", C.c_double), ("sum2_ms", C.c_double), ("sweep_ms", C.c_double), ("cross_ms", C.c_double)]


CORSTRS = {"independence": 0, "exchangeable": 1}  # enum sglm_corstr


class GeeOpts(C.Structure):
    _fields_ = [("corstr", C.c_int), ("fix_rho", C.c_int), ("rho", C.c_double)]


class GeeInfo(C.Structure):
    _fields_ = [("rho", C.c_double), ("phi", C.c_double), ("N", C.c_double), ("G_eff", C.c_int32),
                ("n_max", C.c_int32), ("rows_ms", C.c_double), ("sum_ms", C.c_double), ("combine_ms", C.c_double),
                ("gram_ms", C.c_double)]


# the (family, link) pairs of a Firth fit: the phi = 1 families
FIRTH_LINKS = {"binomial": ("logit", "probit", "cloglog"), "poisson": ("log", "identity", "sqrt")}


class FirthOpts(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("maxit", C.c_int), ("max_halvings", C.c_int)]


class FirthInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("halvings", C.c_int), ("deviance", C.c_double),
                ("pen_deviance", C.c_double), ("logdet", C.c_double), ("score_inf", C.c_double),
                ("sum_hat", C.c_double), ("firth_ms", C.c_double), ("pass_ms", C.c_double)]


MULTINOM_MAX_K, MULTINOM_MAX_Q = 16, 1024  # classes; (K - 1) p


class MultinomOpts(C.Structure):
    _fields_ = [("n_classes", C.c_int), ("epsilon", C.c_double), ("max_iter", C.c_int), ("max_halvings", C.c_int)]


class MultinomInfo(C.Structure):
    _fields_ = [("iter", C.c_int), ("halvings", C.c_int), ("converged", C.c_int), ("deviance", C.c_double),
                ("null_deviance", C.c_double), ("loglik", C.c_double), ("aic", C.c_double),
                ("score_inf", C.c_double), ("class_weight", C.c_double * 16)]


class PreLM(C.Structure):
    _fields_ = [("coefs", dp), ("xtxi", dp), ("std_err", dp), ("sse", C.c_double), ("r2", C.c_double),
                ("fstat", C.c_double), ("sigma", C.c_double), ("nrow", C.c_double), ("npart", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("passes", C.c_int64), ("pass_kernel_ms", C.c_double), ("reduce_kernel_ms", C.c_double),
                ("last_pass_ms", C.c_double), ("comm_ms", C.c_double), ("solve_ms", C.c_double),
                ("n_local", C.c_int64), ("p", C.c_int64), ("workgroups", C.c_int), ("kernel_variant", C.c_int),
                ("path", C.c_int), ("wide_panels", C.c_int), ("row_kernel_ms", C.c_double),
                ("gram_kernel_ms", C.c_double), ("load_ms", C.c_double), ("load_bytes", C.c_int64),
                ("ndev", C.c_int), ("rccl_group", C.c_int), ("dev_passes", C.c_int64),
                ("overlap_chunks", C.c_int), ("comm_path", C.c_int), ("rank_blocks", C.c_int),
                ("pass_kernel_ms_min", C.c_double), ("proc_chunks", C.c_int), ("proc_chunk_rows", C.c_int64),
                ("solve_path", C.c_int), ("pass_kernel", C.c_int), ("pass_kernel_name", C.c_char * 64),
                ("lm_device_fits", C.c_int64), ("lm_device_reruns", C.c_int64),
                ("lm_onepass_fits", C.c_int64)]


COMM_PATHS = {0: "none", 1: "caller-host", 2: "caller-device", 3: "rccl", 4: "group-rccl", 5: "group-host"}
SOLVE_PATHS = {-1: "none", 0: "host-cholesky", 1: "host-lu", 2: "device-cholesky", 3: "device-lu"}
PASS_KERNELS = {0: "none", 1: "fused", 2: "fused-split", 3: "narrow", 4: "wide", 5: "wide-procedural"}


class GlmDerived(C.Structure):
    _fields_ = [("df_residual", C.c_double), ("df_null", C.c_double), ("p_dispersion", C.c_double),
                ("aic", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_int64, C.c_void_p, C.c_int)
LOCAL_SUMS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp)
PASS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, dp, C.c_double, C.c_double, dp)


class Backend(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("p", C.c_int64), ("local_sums", LOCAL_SUMS_FN), ("pass_", PASS_FN)]


class SGLMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[sglm status {code}] {msg}")
        self.code = code


class CommError(SGLMError):
    """SGLM_ECOMM: the all-reduce failed -- RCCL or caller error, or no completion within
    SGLM_COMM_TIMEOUT_S (a peer rank died or stalled); the message names the rank."""


class IllegalArgumentException(ValueError):
    """The reference's require(...) failures (java.lang.IllegalArgumentException)."""


class MatrixSingularException(ArithmeticError):
    """breeze.linalg.MatrixSingularException raised by inv()."""


_lib = None


def load():
    """Load the in-tree HIP library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"sparkglm_amd: HIP engine library missing at {LIB_PATH}; "
                          f"build it with `make -C sparkglm_amd/csrc` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    E = C.POINTER(C.c_void_p)
    h = C.c_void_p
    sig = {
        "sglm_abi_version": ([], C.c_int),
        "sglm_last_error": ([], C.c_char_p),
        "sglm_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "sglm_create": ([C.POINTER(C.c_int), C.c_int, E], C.c_int),
        "sglm_create_device": ([C.c_int, E], C.c_int),
        "sglm_create_multi": ([C.POINTER(C.c_int), C.c_int, E], C.c_int),
        "sglm_destroy": ([h], None),
        "sglm_set_data": ([h, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, dp], C.c_int),
        "sglm_set_data_device": ([h, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p], C.c_int),
        "sglm_synth": ([h, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_uint64], C.c_int),
        "sglm_synth_procedural": ([h, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_uint64], C.c_int),
        "sglm_get_data": ([h, dp, dp, dp, dp, dp], C.c_int),
        "sglm_set_comm": ([h, ALLREDUCE_FN, C.c_void_p, C.c_int], C.c_int),
        "sglm_set_comm_rank": ([h, C.c_int], C.c_int),
        "sglm_rccl_unique_id": ([C.c_void_p], C.c_int),
        "sglm_set_comm_rccl": ([h, C.c_int, C.c_int, C.c_void_p], C.c_int),
        "sglm_fit_glm": ([h, C.POINTER(GlmOpts), C.POINTER(PreGLM)], C.c_int),
        "sglm_fit_lm": ([h, C.POINTER(PreLM)], C.c_int),
        "sglm_irls_pass": ([h, C.POINTER(GlmOpts), dp, C.c_double, dp, dp, dp], C.c_int),
        "sglm_irls_step": ([h, C.POINTER(GlmOpts), dp, dp, dp, dp], C.c_int),
        "sglm_irls_iterations": ([h, C.POINTER(GlmOpts), dp, C.c_int, dp], C.c_int),
        "sglm_predict": ([h, dp, C.c_int, dp], C.c_int),
        "sglm_get_stats": ([h, C.POINTER(Stats)], C.c_int),
        "sglm_reset_stats": ([h], C.c_int),
        "sglm_fit_glm_external": ([C.POINTER(Backend), ALLREDUCE_FN, C.c_void_p, C.POINTER(GlmOpts),
                                   C.POINTER(PreGLM)], C.c_int),
        "sglm_fit_lm_external": ([C.POINTER(Backend), ALLREDUCE_FN, C.c_void_p, C.POINTER(PreLM)], C.c_int),
        "sglm_glm_create_obj": ([C.POINTER(PreGLM), C.c_int64, C.POINTER(GlmDerived)], C.c_int),
        "sglm_glm_summary": ([C.POINTER(PreGLM), C.c_int64, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p,
                              C.c_char_p, C.c_char_p, C.c_int64], C.c_int64),
        "sglm_lm_summary": ([C.POINTER(PreLM), C.c_int64, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p,
                             C.c_int64], C.c_int64),
        "sglm_sig_digits": ([C.c_double, C.c_int], C.c_double),
        "sglm_round_digits": ([C.c_double, C.c_int], C.c_double),
        "sglm_java_double_string": ([C.c_double, C.c_char_p, C.c_int64], C.c_int64),
        "sglm_pval_normal": ([C.c_double], C.c_double),
        "sglm_pval_t": ([C.c_double, C.c_double], C.c_double),
        "sglm_handle_devices": ([h, C.POINTER(C.c_int)], C.c_int),
        "sglm_reserve": ([h, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int], C.c_int),
        "sglm_set_rows": ([h, C.c_int64, C.c_int64, dp, C.c_int64, dp, dp, dp, dp], C.c_int),
        "sglm_predict_glm": ([h, dp, C.c_int, C.c_int, C.c_int, C.c_int, dp], C.c_int),
        "sglm_predict_new": ([h, dp, C.c_int64, C.c_int64, C.c_int64, dp, dp, dp, C.c_int, C.c_int, C.c_int, dp],
                             C.c_int),
        "sglm_local_comm_create": ([C.c_int, C.POINTER(C.c_void_p)], C.c_int),
        "sglm_local_comm_destroy": ([C.c_void_p], None),
        "sglm_local_comm_rank": ([C.c_void_p, C.c_int], C.c_void_p),
        "sglm_local_allreduce": ([C.c_void_p, dp, C.c_int64, C.c_void_p, C.c_int], C.c_int),
        "sglm_pass_kernel_for": ([C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int64],
                                 C.c_int),
        "sglm_vcov": ([h, C.POINTER(GlmOpts), dp, dp], C.c_int),
        "sglm_influence": ([h, C.POINTER(GlmOpts), dp, C.c_int, C.c_double, dp, dp, dp, dp], C.c_int),
        "sglm_predict_new_se": ([h, dp, C.c_int64, C.c_int64, C.c_int64, dp, C.c_double, dp], C.c_int),
        "sglm_get_influence_ms": ([h, dp], C.c_int),
        "sglm_vcov_robust": ([h, C.POINTER(GlmOpts), dp, C.c_int, dp, dp], C.c_int),
        "sglm_get_sandwich_ms": ([h, dp, dp], C.c_int),
        "sglm_set_clusters": ([h, C.POINTER(C.c_int32), C.c_int64, C.c_int32], C.c_int),
        "sglm_vcov_cluster": ([h, C.POINTER(GlmOpts), dp, C.c_int, C.c_int, dp, dp], C.c_int),
        "sglm_get_cluster_ms": ([h, dp, dp, dp, dp], C.c_int),
        "sglm_set_theta": ([h, C.c_double], C.c_int),
        "sglm_get_theta": ([h, dp], C.c_int),
        "sglm_get_theta_ms": ([h, C.POINTER(C.c_int64), dp], C.c_int),
        "sglm_nb_theta_terms": ([h, C.POINTER(GlmOpts), dp, C.c_double, dp], C.c_int),
        "sglm_theta_ml": ([h, C.POINTER(GlmOpts), dp, C.c_int, C.c_double, dp, dp, C.POINTER(C.c_int),
                           C.POINTER(C.c_int)], C.c_int),
        "sglm_fit_glm_start": ([h, C.POINTER(GlmOpts), dp, C.POINTER(PreGLM)], C.c_int),
        "sglm_fit_glm_nb": ([h, C.POINTER(GlmOpts), C.POINTER(NbOpts), C.POINTER(PreGLM), C.POINTER(NbResult)],
                            C.c_int),
        "sglm_fit_glm_fe": ([h, C.POINTER(GlmOpts), C.POINTER(PreGLM), dp, C.POINTER(FeInfo)], C.c_int),
        "sglm_fe_pass": ([h, C.POINTER(GlmOpts), dp, dp, dp, dp, dp, dp], C.c_int),
        "sglm_vcov_fe": ([h, C.POINTER(GlmOpts), dp, dp, C.c_int, C.c_int, C.c_int, dp, dp], C.c_int),
        "sglm_get_fe_ms": ([h, dp, dp, dp, dp], C.c_int),
        "sglm_set_fe2": ([h, C.POINTER(C.c_int32), C.c_int64, C.c_int32], C.c_int),
        "sglm_fe2_plan": ([C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.c_int32,
                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)], C.c_int),
        "sglm_fit_glm_fe2": ([h, C.POINTER(GlmOpts), C.POINTER(Fe2Opts), C.POINTER(PreGLM), dp, dp,
                              C.POINTER(Fe2Info)], C.c_int),
        "sglm_fe2_pass": ([h, C.POINTER(GlmOpts), C.POINTER(Fe2Opts), dp, dp, dp, dp, dp, dp, dp, dp, dp,
                           C.POINTER(C.c_int)], C.c_int),
        "sglm_vcov_fe2": ([h, C.POINTER(GlmOpts), C.POINTER(Fe2Opts), dp, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp],
                          C.c_int),
        "sglm_get_fe2_ms": ([h, dp], C.c_int),
        "sglm_fit_glm_gee": ([h, C.POINTER(GlmOpts), C.POINTER(GeeOpts), C.POINTER(PreGLM), C.POINTER(GeeInfo)],
                             C.c_int),
        "sglm_gee_pass": ([h, C.POINTER(GlmOpts), C.POINTER(GeeOpts), dp, dp, dp, dp, dp, dp, dp], C.c_int),
        "sglm_vcov_gee": ([h, C.POINTER(GlmOpts), C.POINTER(GeeOpts), dp, C.c_double, C.c_int, C.c_int, dp, dp],
                          C.c_int),
        "sglm_get_gee_ms": ([h, dp], C.c_int),
        "sglm_fit_glm_firth": ([h, C.POINTER(GlmOpts), C.POINTER(FirthOpts), dp, C.POINTER(PreGLM),
                                C.POINTER(FirthInfo)], C.c_int),
        "sglm_firth_pass": ([h, C.POINTER(GlmOpts), dp, dp, dp, dp, dp], C.c_int),
        "sglm_get_firth_ms": ([h, dp], C.c_int),
        "sglm_multinom_pass": ([h, C.c_int, dp, dp, dp, dp, dp], C.c_int),
        "sglm_fit_multinom": ([h, C.POINTER(MultinomOpts), dp, dp, dp, dp, C.POINTER(MultinomInfo)], C.c_int),
        "sglm_get_multinom_ms": ([h, dp, dp, dp, dp], C.c_int),
        "sglm_cluster_plan": ([C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.POINTER(C.c_int64),
                               C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)], C.c_int),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("SGLM_LIB") and not hasattr(lib, name):
            continue  # an older build under A/B comparison (tools/ab.py)
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = res
    _lib = lib
    return lib


def pass_kernel_for(n: int, p: int, family: str = "binomial", link: str = "logit", fused_split: int = 1,
                    procedural: bool = False, force_wide: bool = False):
    """(kind, name) of the kernel an engine runs an n x p pass with (sglm_pass_kernel_for; no GPU)."""
    buf = C.create_string_buffer(64)
    flags = (1 if procedural else 0) | (2 if force_wide else 0)
    k = load().sglm_pass_kernel_for(int(n), int(p), int(fused_split), flags, FAMILIES[family], LINKS[link], buf, 64)
    if k < 0:
        raise IllegalArgumentException(last_error())
    return PASS_KERNELS[k], buf.value.decode()


CLUSTER_TYPES = ("HC0", "HC1")  # the adjustments sglm_vcov_cluster takes (sandwich::vcovCL)


def cluster_plan(ids, G: int):
    """(tile_rows, seg_start [nseg + 1], seg_cluster [nseg]): the engine's segmentation of rows with
    dense cluster codes `ids` (sglm_cluster_plan; no GPU)."""
    import numpy as np
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    n = ids.shape[0]
    lib = load()
    ip = ids.ctypes.data_as(C.POINTER(C.c_int32)) if n else None
    tile, nseg = C.c_int64(), C.c_int64()
    check(lib.sglm_cluster_plan(ip, n, int(G), C.byref(tile), C.byref(nseg), None, None), "sglm_cluster_plan")
    start, clus = np.zeros(nseg.value + 1, dtype=np.int64), np.zeros(nseg.value, dtype=np.int32)
    check(lib.sglm_cluster_plan(ip, n, int(G), None, None, start.ctypes.data_as(C.POINTER(C.c_int64)),
                                clus.ctypes.data_as(C.POINTER(C.c_int32))), "sglm_cluster_plan")
    return tile.value, start, clus


def fe2_plan(ids1, ids2, G: int, H: int):
    """dict(chunk_len, chunk_start [nchunk + 1], chunk_level [nchunk], list [n], ncomp, comp_low [ncomp]): the
    engine's plan for two factors with dense codes (sglm_fe2_plan; no GPU) -- factor 2's rows ordered by code,
    cut into chunks, and the connected components of the level graph with each one's lowest factor-2 code."""
    import numpy as np
    ids1 = np.ascontiguousarray(ids1, dtype=np.int32).reshape(-1)
    ids2 = np.ascontiguousarray(ids2, dtype=np.int32).reshape(-1)
    if ids1.shape != ids2.shape:
        raise IllegalArgumentException("requirement failed: ids1 and ids2 have the same number of rows")
    n = ids1.shape[0]
    lib = load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    clen, nch, ncomp = C.c_int64(), C.c_int64(), C.c_int32()
    check(lib.sglm_fe2_plan(ip(ids1), ip(ids2), n, int(G), int(H), C.byref(clen), C.byref(nch), None, None, None,
                            C.byref(ncomp), None), "sglm_fe2_plan")
    start, level = np.zeros(nch.value + 1, dtype=np.int64), np.zeros(max(nch.value, 1), dtype=np.int32)
    rows, low = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(ncomp.value, 1), dtype=np.int32)
    check(lib.sglm_fe2_plan(ip(ids1), ip(ids2), n, int(G), int(H), None, None, lp(start), ip(level), lp(rows), None,
                            ip(low)), "sglm_fe2_plan")
    return dict(chunk_len=clen.value, chunk_start=start, chunk_level=level[: nch.value], list=rows[:n],
                ncomp=ncomp.value, comp_low=low[: ncomp.value])


def last_error() -> str:
    return (load().sglm_last_error() or b"").decode()


def check(rc: int, what: str = "") -> None:
    if rc == SGLM_OK:
        return
    msg = last_error()
    if rc == SGLM_EINVAL:
        raise IllegalArgumentException(msg)
    if rc == SGLM_ESINGULAR:
        raise MatrixSingularException(msg)
    if rc == SGLM_ECOMM:
        raise CommError(rc, f"{what}: {msg}" if what else msg)
    raise SGLMError(rc, f"{what}: {msg}" if what else msg)


def ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(dp)


def java_double_str(x: float) -> str:
    buf = C.create_string_buffer(64)
    load().sglm_java_double_string(float(x), buf, 64)
    return buf.value.decode()
