"""Python handle over the C ABI: one `Engine` per HIP device (one per rank).

This is plumbing around libsglm_hip.so; every fit runs in the C++ driver and the gfx950
kernels.  See include/sglm.h for the contract of each call.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L


@dataclass
class FitGLM:
    """PreGLM (GLM.scala:25-33) plus the deviance trace."""
    coefs: np.ndarray
    stderr: np.ndarray
    deviance: float
    null_deviance: float
    pearson: float
    loglik: float
    iter: int
    nrow: float
    npart: int
    dev_trace: np.ndarray = field(default=None)


@dataclass
class FitNB:
    """sglm_fit_glm_nb: the last inner negative binomial fit and the estimated theta (MASS::glm.nb)."""
    fit: FitGLM
    theta: float
    se_theta: float
    twologlik: float
    outer_iter: int
    theta_warn: int   # bit 0: theta.ml's iteration limit reached, bit 1: estimate truncated at zero
    converged: bool


@dataclass
class FitFE:
    """sglm_fit_glm_fe: the fit of beta (as sglm_fit_glm's), the fixed effects alpha [G] (NaN: a group without
    weight), the number of groups with weight and df_residual = n - p - G_eff."""
    fit: FitGLM
    alpha: np.ndarray
    G_eff: int
    df_residual: float


@dataclass
class FitGEE:
    """sglm_fit_glm_gee: the fit of beta (stderr: the model-based sqrt(diag(inv(A))), unscaled), rho and the scale
    phi at the returned coefficients, the rows and the groups of positive prior weight, the largest group."""
    fit: FitGLM
    rho: float
    phi: float
    N: float
    G_eff: int
    n_max: int


@dataclass
class FitFirth:
    """sglm_fit_glm_firth: the fit of beta (every field at the returned coefficients; fit.iter: the steps taken),
    whether the step's 1-norm met epsilon, the step halvings, the penalized deviance D - log det(X'WX), log
    det(X'WX), |g*|_inf and sum h."""
    fit: FitGLM
    converged: bool
    halvings: int
    pen_deviance: float
    logdet: float
    score_inf: float
    sum_hat: float


@dataclass
class FitMultinom:
    """sglm_fit_multinom: coefs / stderr as [K - 1, p] tables (row j - 1: class j against the baseline, class 0),
    cov [q, q] = inv(H) over the class-major parameter vector, everything at the returned coefficients."""
    coefs: np.ndarray
    stderr: np.ndarray
    cov: np.ndarray
    deviance: float
    null_deviance: float
    loglik: float
    aic: float
    iter: int
    halvings: int
    converged: bool
    score_inf: float
    class_weight: np.ndarray


@dataclass
class FitFE2:
    """sglm_fit_glm_fe2: the fit of beta, the effects alpha [G] and gamma [H] (NaN: a level without weight;
    gamma is 0 at the lowest factor-2 code of every component), the sweeps (last iteration, total), the levels
    with weight, the components of the level graph and df_residual = n - p - (G_eff + H_eff - ncomp)."""
    fit: FitGLM
    alpha: np.ndarray
    gamma: np.ndarray
    sweeps: tuple
    df_residual: float
    ncomp: int
    G_eff: int
    H_eff: int


@dataclass
class ThetaML:
    """sglm_theta_ml (MASS::theta.ml)."""
    theta: float
    se: float
    iters: int
    warn: int


@dataclass
class FitLM:
    """PreLM (LM.scala:10-14) plus LM.fit's stdErr and sigma (LM.scala:260-263)."""
    coefs: np.ndarray
    xtxi: np.ndarray
    stderr: np.ndarray
    sse: float
    r2: float
    fstat: float
    sigma: float
    nrow: float
    npart: int


@dataclass
class Influence:
    """Per-row diagnostics (R's hatvalues / residuals / cooks.distance) and sum(hat)."""
    hat: np.ndarray
    resid: np.ndarray
    cooks: np.ndarray
    sum_hat: float


def _vec(a, n):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if a.shape[0] != n:
        raise L.IllegalArgumentException("requirement failed: The two DataFrames must have the same number of rows")
    return a


def glm_opts(family="binomial", link="logit", tol=1e-6, verbose=False, max_iter=0, init="single", npart=0):
    fam = family.lower()
    if fam not in L.FAMILIES:
        raise L.IllegalArgumentException(f"requirement failed: unknown family {family!r}")
    if link not in L.LINKS:
        raise L.IllegalArgumentException(f"requirement failed: unknown link {link!r}")
    return L.GlmOpts(L.FAMILIES[fam], L.LINKS[link], float(tol), int(bool(verbose)), int(max_iter),
                     L.INIT_MULTIPLE if init == "multiple" else L.INIT_SINGLE, int(npart))


def gee_opts(corstr="exchangeable", rho=None):
    """sglm_gee_opts: the working correlation and, with `rho` given, its fixed value."""
    if corstr not in L.CORSTRS:
        raise L.IllegalArgumentException(f"requirement failed: corstr must be one of {sorted(L.CORSTRS)}, "
                                         f"got {corstr!r}")
    if rho is not None and not (np.isfinite(rho) and rho < 1.0):
        raise L.IllegalArgumentException(f"requirement failed: a fixed rho is finite and below 1 (got {rho!r})")
    return L.GeeOpts(L.CORSTRS[corstr], int(rho is not None), 0.0 if rho is None else float(rho))


class Engine:
    """One HIP device holding one row shard of the design in HBM (SURVEY 8(b)'s constructor
    sglm_create(const int* devs, int ndev = 1)) -- or, with `devices=[...]`, the group handle over
    those devices (sglm_create_multi: row shards per device, one RCCL group all-reduce per
    iteration, for one listed device too; a device listed twice shares the card and sums on the
    host)."""

    def __init__(self, device: int = 0, devices=None):
        self._lib = L.load()
        h = C.c_void_p()
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            L.check(self._lib.sglm_create_multi(devs, len(devices), C.byref(h)), "sglm_create_multi")
            device = int(devices[0])
        else:
            one = (C.c_int * 1)(int(device))
            L.check(self._lib.sglm_create(one, 1, C.byref(h)), "sglm_create")
        self._h = h
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self.n = 0
        self.p = 0
        self._comm_keep = None

    # ---- lifecycle ----
    def close(self):
        if getattr(self, "_h", None):
            self._lib.sglm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- data ----
    def set_data(self, X, y, m=None, offset=None, prior=None):
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise L.IllegalArgumentException("requirement failed: X must be a matrix")
        n, p = X.shape
        y, m, offset, prior = _vec(y, n), _vec(m, n), _vec(offset, n), _vec(prior, n)
        L.check(self._lib.sglm_set_data(self._h, L.ptr(X), n, p, n, L.ptr(y), L.ptr(m), L.ptr(offset),
                                        L.ptr(prior)), "sglm_set_data")
        self.n, self.p = n, p
        return self

    def reserve(self, n: int, p: int, m=False, offset=False, prior=False):
        """Allocate the resident shard; rows then arrive by set_rows (partition-wise ingest)."""
        L.check(self._lib.sglm_reserve(self._h, int(n), int(p), int(bool(m)), int(bool(offset)), int(bool(prior))),
                "sglm_reserve")
        self.n, self.p = int(n), int(p)
        return self

    def set_rows(self, row0: int, X, y, m=None, offset=None, prior=None):
        """Rows [row0, row0 + len(y)) of the reserved shard (one Spark partition's block)."""
        X = np.asfortranarray(X, dtype=np.float64)
        nr = X.shape[0]
        y, m, offset, prior = _vec(y, nr), _vec(m, nr), _vec(offset, nr), _vec(prior, nr)
        L.check(self._lib.sglm_set_rows(self._h, int(row0), nr, L.ptr(X), max(nr, 1), L.ptr(y), L.ptr(m),
                                        L.ptr(offset), L.ptr(prior)), "sglm_set_rows")
        return self

    def set_data_device(self, X, y, m=None, offset=None, prior=None):
        """Torch tensors already on this engine's device: X (n, p) column-major (stride(0) == 1,
        e.g. X.t().contiguous().t()), y / m / offset / prior contiguous length-n vectors, all
        float64.  The engine copies n doubles from every pointer, so anything else is refused
        here rather than read past its allocation."""
        import torch
        if X.dim() != 2:
            raise L.IllegalArgumentException("requirement failed: X must be a matrix")
        n, p = X.shape
        ldx = X.stride(1)
        dev = torch.device("cuda", self.device)

        def _ok(t, what):
            if t.dtype != torch.float64:
                raise L.IllegalArgumentException(f"requirement failed: {what} must be float64, got {t.dtype}")
            if not t.is_cuda or t.device != dev:
                raise L.IllegalArgumentException(f"requirement failed: {what} must live on {dev}, got {t.device}")

        _ok(X, "X")
        if X.stride(0) != 1 or (p > 1 and ldx < n):
            raise L.IllegalArgumentException("requirement failed: X must be column-major on device (stride(0) == 1, "
                                             "leading dimension >= n)")
        for t, what in ((y, "y"), (m, "m"), (offset, "offset"), (prior, "prior")):
            if t is None:
                continue
            _ok(t, what)
            if tuple(t.shape) not in ((n,), (n, 1)) or (n > 1 and t.stride(0) != 1):
                raise L.IllegalArgumentException(f"requirement failed: {what} must be a contiguous vector of "
                                                 f"length {n}")
        ldx = max(ldx, n) if p == 1 else ldx
        g = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        L.check(self._lib.sglm_set_data_device(self._h, g(X), n, p, ldx, g(y), g(m), g(offset), g(prior)),
                "sglm_set_data_device")
        self.n, self.p = n, p
        return self

    def synth(self, kind: int, row0: int, n: int, p: int, seed: int, procedural: bool = False):
        """Rows [row0, row0+n) of the seeded synthetic design generated in HBM.  procedural=True
        stores y (+ offset / prior) only and regenerates X inside the kernels (wide path)."""
        fn = self._lib.sglm_synth_procedural if procedural else self._lib.sglm_synth
        L.check(fn(self._h, int(kind), int(row0), int(n), int(p), C.c_uint64(seed & (2**64 - 1))),
                "sglm_synth_procedural" if procedural else "sglm_synth")
        self.n, self.p = n, p
        return self

    def get_data(self):
        X = np.empty((self.n, self.p), order="F")
        y, m, off, pr = (np.empty(self.n) for _ in range(4))
        L.check(self._lib.sglm_get_data(self._h, L.ptr(X), L.ptr(y), L.ptr(m), L.ptr(off), L.ptr(pr)))
        return X, y, m, off, pr

    # ---- communicators ----
    def set_comm(self, fn, on_device: bool, rank=None):
        """fn(buf_ptr:int, count:int, stream:int, on_device:bool) -> None, sums in place.  With
        `rank` (this process's rank in fn's group) the scalars are summed in rank order with
        compensation (sglm_set_comm_rank)."""
        def _cb(ctx, buf, count, stream, dev):
            try:
                fn(C.cast(buf, C.c_void_p).value, int(count), stream, bool(dev))
                return 0
            except Exception:  # an exception cannot cross the C frame
                import traceback
                traceback.print_exc()
                return 1
        cb = L.ALLREDUCE_FN(_cb)
        self._comm_keep = cb
        L.check(self._lib.sglm_set_comm(self._h, cb, None, int(bool(on_device))), "sglm_set_comm")
        if rank is not None:
            L.check(self._lib.sglm_set_comm_rank(self._h, int(rank)), "sglm_set_comm_rank")

    def set_comm_local(self, rank):
        """Join an in-process communicator (distributed.LocalComm(n).rank(r)): host threads of
        one process, one engine each."""
        self._comm_keep = rank
        L.check(self._lib.sglm_set_comm(self._h, rank.comm.fn, C.c_void_p(rank.ctx), 0), "sglm_set_comm")

    def set_comm_rccl(self, nranks: int, rank: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(self._lib.sglm_set_comm_rccl(self._h, int(nranks), int(rank), buf), "sglm_set_comm_rccl")

    @staticmethod
    def rccl_unique_id() -> bytes:
        lib = L.load()
        buf = C.create_string_buffer(128)
        L.check(lib.sglm_rccl_unique_id(buf), "sglm_rccl_unique_id")
        return buf.raw

    # ---- fits ----
    def fit_glm(self, family="binomial", link="logit", tol=1e-6, verbose=False, max_iter=0, init="single",
                npart=0, max_trace=512, start=None) -> FitGLM:
        """`start` (R's start=): coefficients the iterations begin at (sglm_fit_glm_start); dev_trace[0] is
        then the deviance at `start`.  family "negbin" fits at the handle's theta (set_theta)."""
        o = glm_opts(family, link, tol, verbose, max_iter, init, npart)
        pre, fit = self._pre(max_trace)
        if start is None:
            L.check(self._lib.sglm_fit_glm(self._h, C.byref(o), C.byref(pre)), "sglm_fit_glm")
        else:
            b = self._beta(start)
            L.check(self._lib.sglm_fit_glm_start(self._h, C.byref(o), L.ptr(b), C.byref(pre)), "sglm_fit_glm_start")
        return fit()

    def _pre(self, max_trace):
        """The PreGLM a fit writes, over fresh arrays, and the function that makes its FitGLM after the fit."""
        coefs, se, trace = np.zeros(self.p), np.zeros(self.p), np.full(max_trace, np.nan)
        pre = L.PreGLM(L.ptr(coefs), L.ptr(se), 0, 0, 0, 0, 0, 0, 0, L.ptr(trace), max_trace)
        return pre, lambda: FitGLM(coefs, se, pre.deviance, pre.null_deviance, pre.pearson, pre.loglik, pre.iter,
                                   pre.nrow, pre.npart, trace[: pre.iter + 1].copy())

    def _cov_meat(self, return_meat, name, call):
        """cov, or (cov, meat), of the covariance entry point `name`: call(cov pointer, meat pointer or None)."""
        cov = np.zeros((self.p, self.p), order="F")
        meat = np.zeros((self.p, self.p), order="F") if return_meat else None
        L.check(call(cov.ctypes.data_as(L.dp), None if meat is None else meat.ctypes.data_as(L.dp)), name)
        return (cov, meat) if return_meat else cov

    def _beta(self, beta, p=None):
        """beta as a contiguous vector of p (default: the resident design's) coefficients."""
        p = self.p if p is None else p
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        if b.shape[0] != p:
            raise L.IllegalArgumentException(f"requirement failed: Dimension mismatch: X has {p} columns, "
                                             f"beta {b.shape[0]} rows")
        return b

    # ---- negative binomial ----
    def set_theta(self, theta: float):
        """theta of the "negbin" family on this handle (sglm_set_theta): V = mu + mu^2 / theta."""
        L.check(self._lib.sglm_set_theta(self._h, float(theta)), "sglm_set_theta")
        return self

    def get_theta(self) -> float:
        t = C.c_double()
        L.check(self._lib.sglm_get_theta(self._h, C.byref(t)), "sglm_get_theta")
        return t.value

    def theta_ms(self):
        """(launches, summed kernel ms) of the theta kernel on this handle (HIP events)."""
        k, ms = C.c_int64(), C.c_double()
        L.check(self._lib.sglm_get_theta_ms(self._h, C.byref(k), C.byref(ms)), "sglm_get_theta_ms")
        return k.value, ms.value

    def theta_terms(self, beta, theta: float, link="log") -> np.ndarray:
        """[score, info, loglik, sum w (y/mu - 1)^2, sum w] of the negative binomial's theta at beta."""
        o = glm_opts("negbin", link)
        out = np.zeros(5)
        L.check(self._lib.sglm_nb_theta_terms(self._h, C.byref(o), L.ptr(self._beta(beta)), float(theta), L.ptr(out)),
                "sglm_nb_theta_terms")
        return out

    def theta_ml(self, beta, link="log", limit=0, eps=0.0) -> ThetaML:
        """MASS::theta.ml at beta (limit 0: 25, eps 0: 2^-13)."""
        o = glm_opts("negbin", link)
        th, se, it, warn = C.c_double(), C.c_double(), C.c_int(), C.c_int()
        L.check(self._lib.sglm_theta_ml(self._h, C.byref(o), L.ptr(self._beta(beta)), int(limit), float(eps),
                                        C.byref(th), C.byref(se), C.byref(it), C.byref(warn)), "sglm_theta_ml")
        return ThetaML(th.value, se.value, it.value, warn.value)

    def fit_glm_nb(self, link="log", tol=1e-6, init="single", npart=0, maxit=0, epsilon=0.0, theta_limit=0,
                   theta_eps=0.0, max_iter=0, max_trace=512) -> FitNB:
        """MASS::glm.nb (sglm_fit_glm_nb): theta by maximum likelihood, alternating with negative binomial
        fits; theta stays set on the handle.  Zeros take the defaults 25 / 1e-8 / 25 / 2^-13."""
        o = glm_opts("negbin", link, tol, False, max_iter, init, npart)
        nbo = L.NbOpts(int(maxit), float(epsilon), int(theta_limit), float(theta_eps))
        pre, fit = self._pre(max_trace)
        res = L.NbResult()
        L.check(self._lib.sglm_fit_glm_nb(self._h, C.byref(o), C.byref(nbo), C.byref(pre), C.byref(res)),
                "sglm_fit_glm_nb")
        return FitNB(fit(), res.theta, res.se_theta, res.twologlik, res.outer_iter, res.theta_warn, bool(res.converged))

    def fit_lm(self) -> FitLM:
        p = self.p
        coefs, se, xtxi = np.zeros(p), np.zeros(p), np.zeros((p, p), order="F")
        pre = L.PreLM(L.ptr(coefs), xtxi.ctypes.data_as(L.dp), L.ptr(se), 0, 0, 0, 0, 0, 0)
        L.check(self._lib.sglm_fit_lm(self._h, C.byref(pre)), "sglm_fit_lm")
        return FitLM(coefs, xtxi, se, pre.sse, pre.r2, pre.fstat, pre.sigma, pre.nrow, pre.npart)

    def irls_pass(self, beta=None, mu0=0.0, family="binomial", link="logit", init="single"):
        o = glm_opts(family, link, init=init)
        p = self.p
        gram, xtwz, s = np.zeros((p, p), order="F"), np.zeros(p), np.zeros(L.NS)
        b = None if beta is None else np.ascontiguousarray(beta, dtype=np.float64)
        L.check(self._lib.sglm_irls_pass(self._h, C.byref(o), L.ptr(b), float(mu0), gram.ctypes.data_as(L.dp),
                                         L.ptr(xtwz), L.ptr(s)), "sglm_irls_pass")
        return gram, xtwz, s

    def irls_step(self, beta, family="binomial", link="logit"):
        """SURVEY 8(b)'s test-level step: X'WX, X'Wz and the deviance at beta."""
        o = glm_opts(family, link)
        p = self.p
        xtwx, xtwz, dev = np.zeros((p, p), order="F"), np.zeros(p), C.c_double()
        b = np.ascontiguousarray(beta, dtype=np.float64)
        L.check(self._lib.sglm_irls_step(self._h, C.byref(o), L.ptr(b), xtwx.ctypes.data_as(L.dp), L.ptr(xtwz),
                                         C.byref(dev)), "sglm_irls_step")
        return xtwx, xtwz, dev.value

    def irls_iterations(self, beta, iters, family="binomial", link="logit"):
        o = glm_opts(family, link)
        b = np.ascontiguousarray(beta, dtype=np.float64).copy()
        dev = C.c_double()
        L.check(self._lib.sglm_irls_iterations(self._h, C.byref(o), L.ptr(b), int(iters), C.byref(dev)),
                "sglm_irls_iterations")
        return b, dev.value

    def predict(self, beta, add_offset=False):
        b = np.ascontiguousarray(beta, dtype=np.float64)
        out = np.empty(self.n)
        L.check(self._lib.sglm_predict(self._h, L.ptr(b), int(bool(add_offset)), L.ptr(out)), "sglm_predict")
        return out

    def predict_glm(self, beta, family="binomial", link="logit", type="response", add_offset=True):
        """Fitted values of the resident rows on the link or response scale."""
        o = glm_opts(family, link)
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        out = np.empty(self.n)
        L.check(self._lib.sglm_predict_glm(self._h, L.ptr(b), o.family, o.link, _ptype(type), int(bool(add_offset)),
                                           L.ptr(out)), "sglm_predict_glm")
        return out

    def predict_new(self, X, beta, family="gaussian", link="identity", type="link", offset=None, m=None):
        """Score new rows without touching the resident shard (LM.predict; GLM response scale)."""
        o = glm_opts(family, link)
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise L.IllegalArgumentException("requirement failed: X must be a matrix")
        n, p = X.shape
        b = self._beta(beta, p)
        offset, m = _vec(offset, n), _vec(m, n)
        out = np.empty(n)
        L.check(self._lib.sglm_predict_new(self._h, L.ptr(X), n, p, max(n, 1), L.ptr(b), L.ptr(offset), L.ptr(m),
                                           o.family, o.link, _ptype(type), L.ptr(out)), "sglm_predict_new")
        return out

    # ---- per-row diagnostics ----
    def vcov(self, beta, family="binomial", link="logit"):
        """Unscaled covariance inv(X'WX) at beta (p x p): one pass and the fit's solve rule."""
        o = glm_opts(family, link)
        b = self._beta(beta)
        cov = np.zeros((self.p, self.p), order="F")
        L.check(self._lib.sglm_vcov(self._h, C.byref(o), L.ptr(b), cov.ctypes.data_as(L.dp)), "sglm_vcov")
        return cov

    def influence(self, beta, family="binomial", link="logit", resid="deviance", dispersion=1.0) -> Influence:
        """Leverage, residuals of type `resid` ("deviance" | "pearson" | "working" | "response", on the
        count scale: divide binomial residuals by m for R's proportions), Cook's distance and sum(hat)
        of the resident rows at beta."""
        if resid not in L.RESID_TYPES:
            raise L.IllegalArgumentException(f"requirement failed: resid must be one of {sorted(L.RESID_TYPES)}, "
                                             f"got {resid!r}")
        o = glm_opts(family, link)
        b = self._beta(beta)
        hat, res, cooks = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        sh = C.c_double()
        L.check(self._lib.sglm_influence(self._h, C.byref(o), L.ptr(b), L.RESID_TYPES[resid], float(dispersion),
                                         L.ptr(hat), L.ptr(res), L.ptr(cooks), C.byref(sh)), "sglm_influence")
        return Influence(hat, res, cooks, sh.value)

    def residuals(self, beta, family="binomial", link="logit", resid="deviance"):
        """Residuals only (no covariance product in the kernel)."""
        if resid not in L.RESID_TYPES:
            raise L.IllegalArgumentException(f"requirement failed: resid must be one of {sorted(L.RESID_TYPES)}, "
                                             f"got {resid!r}")
        o = glm_opts(family, link)
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        res = np.empty(self.n)
        L.check(self._lib.sglm_influence(self._h, C.byref(o), L.ptr(b), L.RESID_TYPES[resid], 1.0, None, L.ptr(res),
                                         None, None), "sglm_influence")
        return res

    def predict_new_se(self, X, cov, dispersion=1.0):
        """se.fit on the link scale of new rows: sqrt(dispersion * x' cov x), cov from vcov() / xtxi."""
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise L.IllegalArgumentException("requirement failed: X must be a matrix")
        n, p = X.shape
        cov = np.asfortranarray(cov, dtype=np.float64)
        if cov.shape != (p, p):
            raise L.IllegalArgumentException(f"requirement failed: Dimension mismatch: X has {p} columns, "
                                             f"cov is {cov.shape}")
        out = np.empty(n)
        L.check(self._lib.sglm_predict_new_se(self._h, L.ptr(X), n, p, max(n, 1), cov.ctypes.data_as(L.dp),
                                              float(dispersion), L.ptr(out)), "sglm_predict_new_se")
        return out

    def vcov_robust(self, beta, family="binomial", link="logit", type="HC3", return_meat=False):
        """Heteroskedasticity-consistent covariance C M C at beta (p x p; sandwich::vcovHC types
        "HC0".."HC3"): the bread C = vcov(beta), the meat M = X' diag(omega) X from the score-weight
        kernel and a Gram pass.  It is the final covariance (the dispersion cancels).  With
        `return_meat` the pair (V, M)."""
        if type not in L.HC_TYPES:
            raise L.IllegalArgumentException(f"requirement failed: type must be one of {sorted(L.HC_TYPES)}, "
                                             f"got {type!r}")
        o = glm_opts(family, link)
        b = self._beta(beta)
        return self._cov_meat(return_meat, "sglm_vcov_robust", lambda cov, meat: self._lib.sglm_vcov_robust(
            self._h, C.byref(o), L.ptr(b), L.HC_TYPES[type], cov, meat))

    def sandwich_ms(self):
        """Kernel times (score kernel, meat pass) of the last vcov_robust() call (HIP events)."""
        a, b = C.c_double(), C.c_double()
        L.check(self._lib.sglm_get_sandwich_ms(self._h, C.byref(a), C.byref(b)), "sglm_get_sandwich_ms")
        return a.value, b.value

    # ---- cluster-robust covariance ----
    def set_clusters(self, ids, G=None):
        """The cluster of every resident row (sglm_set_clusters).  With `G=None` the labels -- any
        integer or string dtype -- are factorised (np.unique); with `G` given, `ids` are dense codes in
        [0, G): the form the ranks of a communicator need, so that codes are global.  `ids=None`
        clears.  A call that replaces the data (set_data, reserve, synth, ...) drops the clusters."""
        self._nfe2 = 0  # replacing or clearing the clusters drops the second factor (set_fe2)
        if ids is None:
            L.check(self._lib.sglm_set_clusters(self._h, None, 0, 0), "sglm_set_clusters")
            self._nclusters = 0
            return self
        codes, G = _codes(ids, G, "G", "cluster id")
        L.check(self._lib.sglm_set_clusters(self._h, codes.ctypes.data_as(C.POINTER(C.c_int32)), codes.shape[0], G),
                "sglm_set_clusters")
        self._nclusters = G  # the length of the fixed-effects calls' alpha
        return self

    def vcov_cluster(self, beta, family="binomial", link="logit", type="HC1", cadjust=True, return_meat=False):
        """Cluster-robust covariance a C M C at beta (p x p; sandwich::vcovCL): the bread C = vcov(beta),
        the meat M = S'S of the cluster sums S[g] = sum_{i in g} u_i x_i (set_clusters first).  `type`
        "HC0" | "HC1" ((n - 1) / (n - p)); `cadjust` a further G / (G - 1).  The defaults are vcovCL's
        and Stata's regress, vce(cluster); "HC0" with cadjust is Stata's glm rule.  With `return_meat`
        the pair (V, M)."""
        _cluster_type(type)
        o = glm_opts(family, link)
        b = self._beta(beta)
        return self._cov_meat(return_meat, "sglm_vcov_cluster", lambda cov, meat: self._lib.sglm_vcov_cluster(
            self._h, C.byref(o), L.ptr(b), L.HC_TYPES[type], int(bool(cadjust)), cov, meat))

    def cluster_ms(self):
        """Kernel times (score, segment sums, combine, the meat's Gram pass) of the last vcov_cluster()
        call (HIP events)."""
        t = [C.c_double() for _ in range(4)]
        L.check(self._lib.sglm_get_cluster_ms(self._h, *[C.byref(v) for v in t]), "sglm_get_cluster_ms")
        return tuple(v.value for v in t)

    # ---- one-way fixed effects over the factor of set_clusters ----
    def fit_glm_fe(self, family="poisson", link="log", tol=1e-6, verbose=False, max_iter=0, init="single",
                   npart=0, max_trace=512) -> FitFE:
        """The GLM with one fixed effect per cluster of set_clusters, absorbed (sglm_fit_glm_fe;
        fixest::feglm): every iterate is that of fit_glm on [X | dummies].  X holds no intercept."""
        o = glm_opts(family, link, tol, verbose, max_iter, init, npart)
        pre, fit = self._pre(max_trace)
        alpha = np.zeros(max(self._G(), 1))
        info = L.FeInfo()
        L.check(self._lib.sglm_fit_glm_fe(self._h, C.byref(o), C.byref(pre), L.ptr(alpha), C.byref(info)),
                "sglm_fit_glm_fe")
        return FitFE(fit(), alpha[: self._G()], info.G_eff, info.df_residual)

    def _G(self) -> int:
        return int(getattr(self, "_nclusters", 0))

    def _effects(self, v, name):
        """alpha [G] or gamma [H] as a float64 vector of the declared length."""
        a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        want, what = (self._G(), "clusters (set_clusters)") if name == "alpha" else (self._H(), "levels (set_fe2)")
        if a.shape[0] != want:
            raise L.IllegalArgumentException(f"requirement failed: {name} has {a.shape[0]} entries for {want} {what}")
        return a

    def fe_pass(self, beta=None, alpha=None, family="poisson", link="log", init="single", sums=True):
        """One fixed-effects step at (beta, alpha) (sglm_fe_pass): A, b, the group sums s [G x p], t [G],
        W [G] and the pass's scalars.  beta=None: the initial mode at mean(y) (alpha=None: zeros).
        sums=False: (A, b, scalars) only -- the G (p + 2) group sums are not copied to the host."""
        o = glm_opts(family, link, init=init)
        p, G = self.p, self._G()
        A, b, s = np.zeros((p, p), order="F"), np.zeros(p), np.zeros(L.NS)
        grp = np.zeros(max(G, 1) * (p + 2)) if sums else None
        bb = None if beta is None else self._beta(beta)
        aa = None if alpha is None else self._effects(alpha, "alpha")
        L.check(self._lib.sglm_fe_pass(self._h, C.byref(o), L.ptr(bb), L.ptr(aa), A.ctypes.data_as(L.dp), L.ptr(b),
                                       L.ptr(grp), L.ptr(s)), "sglm_fe_pass")
        if not sums:
            return A, b, s
        S = grp[: G * p].reshape((G, p), order="F")
        return A, b, S, grp[G * p: G * (p + 1)].copy(), grp[G * (p + 1): G * (p + 2)].copy(), s

    def vcov_fe(self, beta, alpha, family="poisson", link="log", cluster=True, type="HC1", cadjust=True,
                return_meat=False):
        """The covariance of beta at (beta, alpha) of a fixed-effects fit (sglm_vcov_fe): inv(A) with
        cluster=False, else clustered on the absorbed factor -- the beta block of sandwich::vcovCL on the
        dummy fit (`type` "HC0" | "HC1" with p + G_eff regressors, `cadjust`)."""
        if cluster:
            _cluster_type(type)
        o = glm_opts(family, link)
        b, a = self._beta(beta), self._effects(alpha, "alpha")
        return self._cov_meat(return_meat, "sglm_vcov_fe", lambda cov, meat: self._lib.sglm_vcov_fe(
            self._h, C.byref(o), L.ptr(b), L.ptr(a), int(bool(cluster)), L.HC_TYPES.get(type, 0), int(bool(cadjust)),
            cov, meat))

    def fe_ms(self):
        """Kernel times (weights, segment sums, combine, the Gram pass over the group sums) of the last
        fixed-effects step (HIP events)."""
        t = [C.c_double() for _ in range(4)]
        L.check(self._lib.sglm_get_fe_ms(self._h, *[C.byref(v) for v in t]), "sglm_get_fe_ms")
        return tuple(v.value for v in t)

    # ---- GEE: an exchangeable working correlation over the factor of set_clusters ----
    def fit_glm_gee(self, family="poisson", link="log", corstr="exchangeable", rho=None, tol=1e-6, verbose=False,
                    max_iter=0, init="single", npart=0, max_trace=512) -> FitGEE:
        """The population-averaged GLM by generalized estimating equations (sglm_fit_glm_gee;
        geepack::geeglm): corstr "exchangeable" (rho estimated by moments at every step, or fixed at `rho`) or
        "independence" (every iterate is fit_glm's).  fit.stderr is the model-based sqrt(diag(inv(A))), unscaled;
        vcov_gee has the robust covariance."""
        o = glm_opts(family, link, tol, verbose, max_iter, init, npart)
        g = gee_opts(corstr, rho)
        pre, fit = self._pre(max_trace)
        info = L.GeeInfo()
        L.check(self._lib.sglm_fit_glm_gee(self._h, C.byref(o), C.byref(g), C.byref(pre), C.byref(info)),
                "sglm_fit_glm_gee")
        return FitGEE(fit(), info.rho, info.phi, info.N, info.G_eff, info.n_max)

    def gee_pass(self, beta=None, family="poisson", link="log", corstr="exchangeable", rho=None, init="single",
                 sums=True):
        """One GEE step at beta (sglm_gee_pass): dict(A, b, s [G x p], t, n, E, Q [G], moments [5] = sum E_g^2,
        sum Q_g, sum n_g (n_g - 1) / 2, N, n_max; scalars, rho).  beta=None: the initial mode, rho = 0.
        sums=False: without s, t, n, E, Q -- the G (p + 4) group sums are not copied to the host."""
        o = glm_opts(family, link, init=init)
        g = gee_opts(corstr, rho)
        p, G = self.p, self._G()
        A, b, s, mom = np.zeros((p, p), order="F"), np.zeros(p), np.zeros(L.NS), np.zeros(5)
        grp = np.zeros(max(G, 1) * (p + 4)) if sums else None
        used = C.c_double()
        bb = None if beta is None else self._beta(beta)
        L.check(self._lib.sglm_gee_pass(self._h, C.byref(o), C.byref(g), L.ptr(bb), A.ctypes.data_as(L.dp), L.ptr(b),
                                        L.ptr(grp), L.ptr(mom), L.ptr(s), C.byref(used)), "sglm_gee_pass")
        if not sums:
            return dict(A=A, b=b, moments=mom, scalars=s, rho=used.value)
        col = lambda k: grp[G * (p + k): G * (p + k + 1)].copy()
        return dict(A=A, b=b, s=grp[: G * p].reshape((G, p), order="F"), t=col(0), n=col(1), E=col(2), Q=col(3),
                    moments=mom, scalars=s, rho=used.value)

    def vcov_gee(self, beta, rho, family="poisson", link="log", corstr="exchangeable", robust=True, cadjust=False,
                 return_meat=False):
        """The covariance of beta at (beta, rho) of a GEE fit (sglm_vcov_gee): robust, inv(A) M inv(A) with the
        meat over the clusters (what geepack / Stata / statsmodels print; `cadjust` a further G / (G - 1)), or
        with robust=False the model-based phi inv(A)."""
        o = glm_opts(family, link)
        g = gee_opts(corstr, None)
        b = self._beta(beta)
        return self._cov_meat(return_meat, "sglm_vcov_gee", lambda cov, meat: self._lib.sglm_vcov_gee(
            self._h, C.byref(o), C.byref(g), L.ptr(b), float(rho), int(bool(robust)), int(bool(cadjust)), cov, meat))

    def gee_ms(self):
        """Kernel times (rows, segment sums, combine, the Gram pass over the group sums) of the last GEE step
        (HIP events)."""
        t = np.zeros(4)
        L.check(self._lib.sglm_get_gee_ms(self._h, L.ptr(t)), "sglm_get_gee_ms")
        return tuple(float(v) for v in t)

    # ---- Firth's bias-reduced fits (binomial, poisson; p <= 256) ----
    def fit_glm_firth(self, family="binomial", link="logit", epsilon=1e-8, maxit=100, start=None, init="single",
                      npart=0, max_trace=512, max_halvings=12, verbose=False) -> FitFirth:
        """Firth's penalized-likelihood fit (sglm_fit_glm_firth; logistf, brglm2's AS_mean): finite under
        separation.  Iterates beta += inv(X'WX) g*(beta) from `start` (default: fit_glm's first iterate) until
        the step's 1-norm is below `epsilon`; converged=False after `maxit` steps is a status, not an error."""
        o = glm_opts(family, link, verbose=verbose, init=init, npart=npart)
        fo = L.FirthOpts(float(epsilon), int(maxit), int(max_halvings))
        pre, fit = self._pre(max_trace)
        info = L.FirthInfo()
        b = None if start is None else self._beta(start)
        L.check(self._lib.sglm_fit_glm_firth(self._h, C.byref(o), C.byref(fo), L.ptr(b), C.byref(pre),
                                             C.byref(info)), "sglm_fit_glm_firth")
        return FitFirth(fit(), bool(info.converged), info.halvings, info.pen_deviance, info.logdet, info.score_inf,
                        info.sum_hat)

    def firth_pass(self, beta, family="binomial", link="logit", hat=False):
        """One Firth pass at beta (sglm_firth_pass): dict(A = X'WX, g = the adjusted score g*, deviance, logdet,
        sum_hat; with hat=True also hat [n], the leverages)."""
        o = glm_opts(family, link)
        b = self._beta(beta)
        A, g, s = np.zeros((self.p, self.p), order="F"), np.zeros(self.p), np.zeros(3)
        hv = np.empty(self.n) if hat else None
        L.check(self._lib.sglm_firth_pass(self._h, C.byref(o), L.ptr(b), A.ctypes.data_as(L.dp), L.ptr(g), L.ptr(hv),
                                          L.ptr(s)), "sglm_firth_pass")
        out = dict(A=A, g=g, deviance=float(s[0]), logdet=float(s[1]), sum_hat=float(s[2]))
        if hat:
            out["hat"] = hv
        return out

    def firth_ms(self) -> float:
        """Kernel time of the last Firth pass (HIP events; -1 before any)."""
        t = C.c_double()
        L.check(self._lib.sglm_get_firth_ms(self._h, C.byref(t)), "sglm_get_firth_ms")
        return t.value

    # ---- multinomial logit (softmax regression; p <= 256, K <= 16, (K - 1) p <= 1024) ----
    def _multinom_B(self, B, K):
        """B as the class-major parameter vector: [p, K - 1] (column j - 1: class j), or already flat."""
        b = np.asarray(B, dtype=np.float64)
        if b.ndim == 2:
            if b.shape != (self.p, K - 1):
                raise L.IllegalArgumentException(f"requirement failed: B is [p, n_classes - 1] = "
                                                 f"[{self.p}, {K - 1}] (got {list(b.shape)})")
            b = b.T
        b = np.ascontiguousarray(b).reshape(-1)
        if K >= 2 and b.shape[0] != (K - 1) * self.p:
            raise L.IllegalArgumentException(f"requirement failed: B has (n_classes - 1) * p = {(K - 1) * self.p} "
                                             f"entries (got {b.shape[0]})")
        return b

    def multinom_pass(self, B, n_classes, prob=False, hessian=True, score=False):
        """One evaluation at B (sglm_multinom_pass): dict(H [q, q], g [q], deviance, sum_w, null_deviance; with
        prob=True also prob [n, K]).  hessian=False: no Gram passes (g with score=True or prob=True); none of the
        three: the deviance-only evaluation."""
        K = int(n_classes)
        b = self._multinom_B(B, K)
        q = max(K - 1, 0) * self.p
        H = np.zeros((q, q), order="F") if hessian else None
        g = np.zeros(q) if hessian or prob or score else None
        pr = np.zeros((self.n, K), order="F") if prob else None
        s = np.zeros(3)
        L.check(self._lib.sglm_multinom_pass(self._h, K, L.ptr(b), L.ptr(H), L.ptr(g), L.ptr(s), L.ptr(pr)),
                "sglm_multinom_pass")
        out = dict(deviance=float(s[0]), sum_w=float(s[1]), null_deviance=float(s[2]))
        if hessian:
            out["H"] = H
        if g is not None:
            out["g"] = g
        if prob:
            out["prob"] = pr
        return out

    def fit_multinom(self, n_classes, epsilon=1e-8, max_iter=100, start=None, max_halvings=12) -> FitMultinom:
        """Newton's method with step halving on the deviance (sglm_fit_multinom) from B = 0 or `start`."""
        K = int(n_classes)
        o = L.MultinomOpts(K, float(epsilon), int(max_iter), int(max_halvings))
        q = max(K - 1, 0) * self.p
        b0 = None if start is None else self._multinom_B(start, K)
        B, se, cov = np.zeros(q), np.zeros(q), np.zeros((q, q), order="F")
        info = L.MultinomInfo()
        L.check(self._lib.sglm_fit_multinom(self._h, C.byref(o), L.ptr(b0), L.ptr(B), L.ptr(se), L.ptr(cov),
                                            C.byref(info)), "sglm_fit_multinom")
        return FitMultinom(B.reshape(K - 1, self.p), se.reshape(K - 1, self.p), cov, info.deviance,
                           info.null_deviance, info.loglik, info.aic, info.iter, info.halvings, bool(info.converged),
                           info.score_inf, np.array(info.class_weight[:K]))

    def multinom_ms(self):
        """Kernel times (rows, X'R, weights, Gram passes) of the last multinomial call (HIP events)."""
        t = [C.c_double() for _ in range(4)]
        L.check(self._lib.sglm_get_multinom_ms(self._h, *[C.byref(v) for v in t]), "sglm_get_multinom_ms")
        return tuple(v.value for v in t)

    # ---- two-way fixed effects: a second factor beside the one of set_clusters ----
    def set_fe2(self, ids, H=None):
        """The second fixed-effects factor of every resident row (sglm_set_fe2), after set_clusters.  With
        `H=None` the labels are factorised (np.unique); with `H` given, `ids` are dense codes in [0, H).
        `ids=None` clears.  Replacing the data or the clusters drops it."""
        if ids is None:
            L.check(self._lib.sglm_set_fe2(self._h, None, 0, 0), "sglm_set_fe2")
            self._nfe2 = 0
            return self
        codes, H = _codes(ids, H, "H", "code of the second factor")
        self._nfe2 = 0
        L.check(self._lib.sglm_set_fe2(self._h, codes.ctypes.data_as(C.POINTER(C.c_int32)), codes.shape[0], H),
                "sglm_set_fe2")
        self._nfe2 = H
        return self

    def _H(self) -> int:
        return int(getattr(self, "_nfe2", 0))

    @staticmethod
    def _fe2_opts(sweep_tol, max_sweeps):
        return L.Fe2Opts(float(sweep_tol), int(max_sweeps))

    def fit_glm_fe2(self, family="poisson", link="log", tol=1e-6, verbose=False, max_iter=0, init="single",
                    npart=0, max_trace=512, sweep_tol=0.0, max_sweeps=0) -> FitFE2:
        """The GLM with one fixed effect per cluster of set_clusters and one per level of set_fe2, both
        absorbed (sglm_fit_glm_fe2; fixest::feglm with two factors): every iterate is that of fit_glm on
        [X | D1 | D2 without one column per component].  X holds no intercept."""
        o = glm_opts(family, link, tol, verbose, max_iter, init, npart)
        fo = self._fe2_opts(sweep_tol, max_sweeps)
        pre, fit = self._pre(max_trace)
        alpha, gamma = np.zeros(max(self._G(), 1)), np.zeros(max(self._H(), 1))
        info = L.Fe2Info()
        L.check(self._lib.sglm_fit_glm_fe2(self._h, C.byref(o), C.byref(fo), C.byref(pre), L.ptr(alpha), L.ptr(gamma),
                                           C.byref(info)), "sglm_fit_glm_fe2")
        return FitFE2(fit(), alpha[: self._G()], gamma[: self._H()], (info.sweeps_last, info.sweeps_total),
                      info.df_residual, info.ncomp, info.G_eff, info.H_eff)

    def fe2_pass(self, beta=None, alpha=None, gamma=None, family="poisson", link="log", init="single",
                 sweep_tol=0.0, max_sweeps=0, sums=True):
        """One two-way step at (beta, alpha, gamma), the sweeps started from zero (sglm_fe2_pass): dict(A, b,
        S1 [G x p], t1, W1, S2 [H x p], t2, W2, Y [(G + H) x (p + 1)], scalars, sweeps).  beta=None: the
        initial mode at mean(y).  sums=False: dict(A, b, scalars, sweeps) only -- the level sums and Y are not
        copied to the host."""
        o = glm_opts(family, link, init=init)
        fo = self._fe2_opts(sweep_tol, max_sweeps)
        p, G, H = self.p, self._G(), self._H()
        A, b, s = np.zeros((p, p), order="F"), np.zeros(p), np.zeros(L.NS)
        g1 = np.zeros(max(G, 1) * (p + 2)) if sums else None
        g2 = np.zeros(max(H, 1) * (p + 2)) if sums else None
        Y = np.zeros((max(G + H, 1), p + 1), order="F") if sums else None
        k = C.c_int()
        bb = None if beta is None else self._beta(beta)
        aa = None if alpha is None else self._effects(alpha, "alpha")
        gg = None if gamma is None else self._effects(gamma, "gamma")
        L.check(self._lib.sglm_fe2_pass(self._h, C.byref(o), C.byref(fo), L.ptr(bb), L.ptr(aa), L.ptr(gg),
                                        A.ctypes.data_as(L.dp), L.ptr(b), L.ptr(g1), L.ptr(g2),
                                        None if Y is None else Y.ctypes.data_as(L.dp), L.ptr(s), C.byref(k)),
                "sglm_fe2_pass")
        if not sums:
            return dict(A=A, b=b, scalars=s, sweeps=k.value)
        out = dict(A=A, b=b, Y=Y, scalars=s, sweeps=k.value)
        for tag, g, n in (("1", g1, G), ("2", g2, H)):
            out["S" + tag] = g[: n * p].reshape((n, p), order="F")
            out["t" + tag] = g[n * p: n * (p + 1)].copy()
            out["W" + tag] = g[n * (p + 1): n * (p + 2)].copy()
        return out

    def vcov_fe2(self, beta, alpha, gamma, family="poisson", link="log", cluster=True, type="HC1", cadjust=True,
                 return_meat=False, sweep_tol=0.0, max_sweeps=0):
        """The covariance of beta at (beta, alpha, gamma) of a two-way fit (sglm_vcov_fe2): inv(A) with
        cluster=False, else clustered on factor 1 -- the beta block of sandwich::vcovCL on the dummy fit."""
        if cluster:
            _cluster_type(type)
        o = glm_opts(family, link)
        fo = self._fe2_opts(sweep_tol, max_sweeps)
        b, a, g = self._beta(beta), self._effects(alpha, "alpha"), self._effects(gamma, "gamma")
        return self._cov_meat(return_meat, "sglm_vcov_fe2", lambda cov, meat: self._lib.sglm_vcov_fe2(
            self._h, C.byref(o), C.byref(fo), L.ptr(b), L.ptr(a), L.ptr(g), int(bool(cluster)), L.HC_TYPES.get(type, 0),
            int(bool(cadjust)), cov, meat))

    def fe2_ms(self):
        """Kernel times (weights, factor-1 sums, factor-2 sums, sweeps, cross product) of the last two-way
        step (HIP events)."""
        t = np.zeros(5)
        L.check(self._lib.sglm_get_fe2_ms(self._h, L.ptr(t)), "sglm_get_fe2_ms")
        return tuple(t)

    def influence_ms(self) -> float:
        """Kernel time of the last influence() call (HIP events)."""
        ms = C.c_double()
        L.check(self._lib.sglm_get_influence_ms(self._h, C.byref(ms)), "sglm_get_influence_ms")
        return ms.value

    def stats(self) -> dict:
        s = L.Stats()
        L.check(self._lib.sglm_get_stats(self._h, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in L.Stats._fields_}
        d["comm_path_name"] = L.COMM_PATHS.get(d["comm_path"], "?")
        d["solve_path_name"] = L.SOLVE_PATHS.get(d["solve_path"], "?")
        d["pass_kernel_name"] = s.pass_kernel_name.decode()
        d["pass_kernel_kind"] = L.PASS_KERNELS.get(d["pass_kernel"], "?")
        return d

    def reset_stats(self):
        L.check(self._lib.sglm_reset_stats(self._h))


def _cluster_type(type):
    if type not in L.CLUSTER_TYPES:
        raise L.IllegalArgumentException(f"requirement failed: with clusters, type must be one of "
                                         f"{list(L.CLUSTER_TYPES)}, got {type!r}")


def _codes(ids, nlev, name, what):
    """(int32 codes, level count) of a factor: labels of any dtype factorised (nlev None), or dense codes checked
    to lie in [0, nlev); `name` / `what`: the count and a code in the caller's messages."""
    ids = np.asarray(ids).reshape(-1)
    if nlev is None:
        labels, ids = np.unique(ids, return_inverse=True)
        nlev = len(labels)
    elif ids.dtype.kind not in "iu":
        raise L.IllegalArgumentException(f"requirement failed: with {name} given, ids are integer codes in [0, {name})")
    elif ids.size and (ids.min() < 0 or ids.max() >= nlev):  # before the cast to int32 can wrap a code
        raise L.IllegalArgumentException(f"requirement failed: every {what} in [0, {name} = {nlev})")
    return np.ascontiguousarray(ids, dtype=np.int32), int(nlev)


def _ptype(t) -> int:
    if t not in ("link", "response"):
        raise L.IllegalArgumentException(f"requirement failed: type must be 'link' or 'response', got {t!r}")
    return L.PREDICT_RESPONSE if t == "response" else L.PREDICT_LINK


def device_count() -> int:
    lib = L.load()
    c = C.c_int()
    rc = lib.sglm_device_count(C.byref(c))
    return c.value if rc == 0 else 0
