"""`GLM` -- the reference's Scala GLM API, over the MI355X engine.

Mirrors com.Alteryx.sparkGLM.GLM (GLM.scala): the sixteen `fit` overloads with their
`require` checks and defaults (tol = 1e-6, m = 1, offset = 0, verbose = false), the
PreGLM / GLM result objects, `createObj` and `summary`.  The fit driver bodies
(fitSingleBinomial / fitMultipleBinomial) are replaced by the engine (sglm_fit_glm).

Faithful-to-the-reference behaviour (``strict = True``, the default):
  * any family string fits binomial unless it names an extension family; binomial links
    are "logit", "probit" and anything else = cloglog (GLM.scala:264-299);
  * only the 4-argument overload runs on a multi-partition DataFrame; every other
    overload requires a single partition ("The DataFrame must be in a single partition",
    utils.scala:43-44) because the reference routes them to fitSingle;
  * fit(y, x, offset, family, link, tol, m) ignores the offset (GLM.scala:789-792);
  * the first iteration uses mu = mean(y) on one partition, unlink(link(mean(y))) on
    several (GLM.scala:263 vs 370-371); npart reports the partition count.
With ``strict = False`` every overload runs on partitioned data and honours its offset.
The extension families "gaussian", "poisson" and "gamma" (R's three links each: identity / log /
inverse, log / identity / sqrt, inverse / identity / log; prior weights through `fit_weighted`)
follow R's family objects on the same IRLS skeleton.  With a non-canonical link a fit whose mean
leaves the family's range raises IllegalArgumentException (no step-halving).  Their `loglik`
is R's logLik; `aic` stays createObj's -2 loglik + 2p (GLM.scala:70), which counts the
coefficients only -- R's AIC(glm) for gaussian and Gamma adds 2 for the dispersion parameter,
so it is 2 higher than `aic` here for those two families.
`GLM.fit_nb` fits the negative binomial (links log / sqrt / identity): with `theta` given it is R's
glm(family = MASS::negative.binomial(theta)), without it MASS::glm.nb, which estimates theta by maximum
likelihood; the model then carries `theta`, `theta_se` and `twologlik`, its dispersion is 1, and its `aic`
counts theta as a parameter when it was estimated (as logLik.negbin does).  `GLM.fit`'s family strings are
unchanged: "negbin" there is an unrecognised family and fits binomial, as the reference does.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib as L
from .engine import Engine
from .frame import Frame

strict = True
_engines = {}


def _engine(device: int = 0) -> Engine:
    e = _engines.get(device)
    if e is None:
        e = _engines[device] = Engine(device)
    return e


def _require(cond: bool, msg: str):
    if not cond:
        raise L.IllegalArgumentException("requirement failed: " + msg)


@dataclass
class PreGLM:
    """GLM.scala:25-33"""
    coefs: np.ndarray
    stdErr: List[float]
    deviance: float
    nullDeviance: float
    pearson: float
    loglik: float
    iter: int
    nrow: float
    npart: int


@dataclass
class GLMModel:
    """The GLM case class (GLM.scala:35-51)."""
    xnames: List[str]
    yname: str
    coefs: np.ndarray
    stdErr: List[float]
    dfResidual: float
    dfNull: float
    deviance: float
    nullDeviance: float
    pDispersion: float
    pearson: float
    loglik: float
    family: str
    link: str
    aic: float
    iter: int
    nrow: float
    npart: int
    # GLM.fit_nb only: the negative binomial's theta (given or estimated), and for MASS::glm.nb fits its
    # standard error and twice the log-likelihood
    theta: Optional[float] = None
    theta_se: Optional[float] = None
    twologlik: Optional[float] = None
    # GLM.fit_fe only: the absorbed factor's effects (label -> alpha; NaN: a group without weight), the groups
    # and rows dropped as uninformative (all y = 0, or all y = m)
    fixef: Optional[dict] = None
    fe_dropped_groups: int = 0
    fe_dropped_rows: int = 0
    # GLM.fit_fe(fe2=) only: the second factor's effects (label -> gamma; 0 at the lowest label of every connected
    # component of the two factors' levels, NaN: a level without weight), the components and the sweeps
    fixef2: Optional[dict] = None
    fe_ncomp: int = 0
    fe_sweeps: Optional[tuple] = None
    # GLM.fit_gee only: the working correlation ("exchangeable" | "independence"), its rho, the scale phi and the
    # model-based standard errors sqrt(phi diag(inv(A))); stdErr holds the robust ones and aic is None
    corstr: Optional[str] = None
    rho: Optional[float] = None
    scale: Optional[float] = None
    naive_se: Optional[List[float]] = None
    # GLM.fit_firth only: the penalized deviance D - log det(X'WX), log det(X'WX), the step halvings and whether
    # the step met epsilon; aic is None (the likelihood is a penalized one)
    pen_deviance: Optional[float] = None
    logdet: Optional[float] = None
    halvings: Optional[int] = None
    converged: Optional[bool] = None

    def predict(self, newData: Frame, type: str = "response", offset: Optional[Frame] = None,
                m: Optional[Frame] = None, device: int = 0, cov=None, dispersion: Optional[float] = None,
                fe: Optional[Frame] = None, fe2: Optional[Frame] = None) -> Frame:
        """Extension (the reference has no GLM predict): (index, value) rows of the
        linear predictor newX * coefs (+ offset) on the "link" scale, or of mu = unlink(eta, m)
        on the "response" scale (m = binomial trials, default 1) -- R's predict.glm(type=).
        Runs on the GPU through sglm_predict_new; newData's columns are taken by the model's
        names.

        With `cov` (the unscaled covariance of GLM.vcov) the frame gains an `se` column, R's
        se.fit: sqrt(dispersion * x' cov x) on the link scale (sglm_predict_new_se), times
        |dmu/deta| on the response scale (the delta method).  `dispersion` defaults to R's rule
        (_dispersion).  Without `cov` the result is unchanged.

        A GLM.fit_fe model takes `fe`, one column with each new row's label of the absorbed factor: the
        label's alpha is added to the offset, and a label the fit has not seen predicts NaN.  A two-way model
        (GLM.fit_fe(fe2=)) takes `fe2` in the same way."""
        _require(len(set(self.xnames) - set(newData.columns)) == 0,
                 "Not all predictors in the estimation data are in the data to be predicted")
        fam, lnk = _model_family_link(self)
        newX = newData.select(*self.xnames).to_matrix()
        beta = np.asarray(self.coefs, dtype=np.float64).reshape(-1)
        off = None if offset is None else offset.to_vector()
        mv = None if m is None else m.to_vector()
        if self.fixef is not None:
            _require(fe is not None and len(fe.columns) == 1, "a fixed-effects model predicts with fe, one column "
                     "of labels")
            _require(fe.count() == newData.count(), "The two DataFrames must have the same number of rows")
            off = fe_offsets(self.fixef, fe[fe.columns[0]], off)
            if self.fixef2 is not None:
                _require(fe2 is not None and len(fe2.columns) == 1 and fe2.count() == newData.count(),
                         "a two-way fixed-effects model predicts with fe2 as well, one column of labels")
                off = fe_offsets(self.fixef2, fe2[fe2.columns[0]], off)
            else:
                _require(fe2 is None, "fe2 belongs to a GLM.fit_fe(fe2=) model")
        else:
            _require(fe is None and fe2 is None, "fe belongs to a GLM.fit_fe model")
        vals = _engine(device).predict_new(newX, beta, fam, lnk, type, off, mv)
        cols = {"index": np.arange(len(vals), dtype=np.int64), "value": vals}
        if cov is not None:
            phi = _dispersion(self) if dispersion is None else float(dispersion)
            se = _engine(device).predict_new_se(newX, cov, phi)
            if type == "response":
                eta = vals if lnk == "identity" else _engine(device).predict_new(newX, beta, fam, lnk, "link", off, mv)
                se = se * np.abs(_dmu_deta(lnk, eta, 1.0 if mv is None else mv))
            cols["se"] = se
        return Frame(cols, newData.npartitions)


def _dispersion(obj) -> float:
    """R's summary.glm rule: 1 for binomial and poisson, the Pearson estimate for gaussian and gamma."""
    fam, _ = _model_family_link(obj)
    return 1.0 if fam in ("binomial", "poisson", "negbin") else float(obj.pDispersion)


def _dmu_deta(link: str, eta, m=1.0):
    """d mu / d eta of mu = unlink(eta, m) for the seven links (the delta method of se.fit)."""
    eta = np.asarray(eta, dtype=np.float64)
    if link == "logit":
        e = np.exp(-np.abs(eta))
        return m * e / (1.0 + e) ** 2
    if link == "probit":
        return m * np.exp(-0.5 * eta * eta) / np.sqrt(2.0 * np.pi)
    if link == "cloglog":
        return m * np.exp(eta - np.exp(eta))
    if link == "identity":
        return np.ones_like(eta)
    if link == "log":
        return np.exp(eta)
    if link == "sqrt":
        return 2.0 * eta
    return -1.0 / (eta * eta)  # inverse


def _engine_family_link(family: str, link: str):
    f = family.lower()
    if f in ("gaussian", "poisson", "gamma"):
        allowed = L.FAMILY_LINKS[f]
        _require(link in allowed, f"family {family} supports only the {', '.join(allowed)} links")
        return f, link
    # binomial, including any unrecognised family string (GLM.scala:486-590)
    if link == "logit":
        return "binomial", "logit"
    if link == "probit":
        return "binomial", "probit"
    return "binomial", "cloglog"


def _model_family_link(obj):
    """The engine's (family, link) of a fitted model: GLM.fit_nb's models are "negbin" (they carry theta);
    every other model goes through GLM.fit's string dispatch."""
    if getattr(obj, "theta", None) is not None and obj.family.lower() == "negbin":
        _require(obj.link in L.NEGBIN_LINKS, f"family negbin supports only the {', '.join(L.NEGBIN_LINKS)} links")
        return "negbin", obj.link
    return _engine_family_link(obj.family, obj.link)


def _nb_summary(text: str, obj, lib) -> str:
    """GLM.summary's text for a GLM.fit_nb model: the AIC line carries obj.aic (which counts theta when it was
    estimated) and a Theta block follows it.  The two anchors are sglm_glm_summary's own lines; if that layout
    ever changes this raises instead of printing a summary without them."""
    aic = "AIC: " + L.java_double_str(lib.sglm_sig_digits(float(obj.aic), 5))
    th = "Theta: " + L.java_double_str(lib.sglm_sig_digits(float(obj.theta), 6))
    if obj.theta_se is not None:
        th += "\nStd. Err.: " + L.java_double_str(lib.sglm_sig_digits(float(obj.theta_se), 6))
        th += "\n2 x log-likelihood: " + L.java_double_str(lib.sglm_sig_digits(float(obj.twologlik), 6))
    text, k = re.subn(r"^AIC: .*$", lambda _: aic + "\n" + th, text, count=1, flags=re.M)
    if k != 1:
        raise RuntimeError("sglm_glm_summary printed no 'AIC: ' line to carry the negative binomial's AIC and theta")
    return text


def _gee_summary(text: str, obj, lib) -> str:
    """GLM.summary's text for a GLM.fit_gee model: there is no likelihood, so the AIC line gives way to the
    working correlation and the scale (the anchor is sglm_glm_summary's own line, as in _nb_summary)."""
    lines = (f"Correlation ({obj.corstr}): " + L.java_double_str(lib.sglm_sig_digits(float(obj.rho), 6)) +
             "\nScale: " + L.java_double_str(lib.sglm_sig_digits(float(obj.scale), 6)))
    text, k = re.subn(r"^AIC: .*$", lambda _: lines, text, count=1, flags=re.M)
    if k != 1:
        raise RuntimeError("sglm_glm_summary printed no 'AIC: ' line to replace with the GEE's correlation and scale")
    return text


def _firth_summary(text: str, obj, lib) -> str:
    """GLM.summary's text for a GLM.fit_firth model: the AIC line gives way to one naming the method and its
    penalized deviance (the anchor is sglm_glm_summary's own line, as in _nb_summary)."""
    line = ("Method: Firth's penalized likelihood (mean bias reduction), penalized deviance: " +
            L.java_double_str(lib.sglm_sig_digits(float(obj.pen_deviance), 6)))
    text, k = re.subn(r"^AIC: .*$", lambda _: line, text, count=1, flags=re.M)
    if k != 1:
        raise RuntimeError("sglm_glm_summary printed no 'AIC: ' line to replace with the Firth fit's method")
    return text


def _check_inputs(y: Frame, x: Frame):
    # GLM.scala:602-609 (identical in every overload)
    _require(all(t == "DoubleType" for _, t in x.dtypes), "The provided DataFrame must contain all 'DoubleType' columns")
    _require(x.rdd.partitions.size() == y.rdd.partitions.size(), "The two DataFrames must have the same number of paritions")
    _require(x.count() == y.count(), "The two DataFrames must have the same number of rows")
    _require(len(y.columns) == 1, "The 'y' DataFrame must have only one column")


def _single_partition(df: Frame):
    # utils.dfToDenseMatrix (utils.scala:43-46)
    _require(df.rdd.partitions.size() == 1, "The DataFrame must be in a single partition")
    _require(all(t == "DoubleType" for _, t in df.dtypes), "The provided DataFrame must contain all 'DoubleType' columns")


def _to_pre(f) -> PreGLM:
    return PreGLM(f.coefs.reshape(-1, 1), list(f.stderr), f.deviance, f.null_deviance, f.pearson, f.loglik, f.iter,
                  f.nrow, f.npart)


def _fit_components(y: Frame, x: Frame, family: str, link: str, tol: float, verbose: bool,
                    offset: Optional[Frame] = None, m: Optional[Frame] = None, prior: Optional[Frame] = None,
                    device: int = 0) -> PreGLM:
    npart = x.rdd.partitions.size()
    fam, lnk = _engine_family_link(family, link)
    for extra in (offset, m, prior):
        if extra is not None:
            if strict or npart == 1:
                _single_partition(extra)
            _require(extra.count() == y.count(), "The two DataFrames must have the same number of rows")
    eng = _engine(device)
    eng.set_data(x.to_matrix(), y.to_vector(), None if m is None else m.to_vector(),
                 None if offset is None else offset.to_vector(), None if prior is None else prior.to_vector())
    f = eng.fit_glm(fam, lnk, tol=tol, verbose=verbose, init="single" if npart == 1 else "multiple", npart=npart)
    return _to_pre(f)


def _pre_struct(pre: PreGLM):
    coefs = np.ascontiguousarray(np.asarray(pre.coefs, dtype=np.float64).reshape(-1))
    se = np.ascontiguousarray(np.asarray(pre.stdErr, dtype=np.float64))
    s = L.PreGLM(L.ptr(coefs), L.ptr(se), pre.deviance, pre.nullDeviance, pre.pearson, pre.loglik, pre.iter,
                 pre.nrow, pre.npart, None, 0)
    return s, (coefs, se)


def _check_cov_type(type):
    if type != "const" and type not in L.HC_TYPES:
        raise L.IllegalArgumentException(f"requirement failed: type must be one of "
                                         f"{['const'] + sorted(L.HC_TYPES)}, got {type!r}")


def _check_cluster_type(type):
    if type not in L.CLUSTER_TYPES:
        raise L.IllegalArgumentException(f"requirement failed: with cluster, type must be one of "
                                         f"{list(L.CLUSTER_TYPES)} (HC2 / HC3 need per-cluster leverage blocks), "
                                         f"got {type!r}")


def _set_clusters(eng, cluster: Frame, n: int):
    """The one column of `cluster` (labels of any integer or string type) as the engine's clusters."""
    _require(len(cluster.columns) == 1, "The 'cluster' DataFrame must have only one column")
    _require(cluster.count() == n, "The two DataFrames must have the same number of rows")
    eng.set_clusters(cluster[cluster.columns[0]])


def _coef_table(names, beta, V, pval) -> Frame:
    """The coeftest columns from a covariance: se = sqrt(diag V), stat = estimate / se, pval(stat)."""
    est = np.asarray(beta, dtype=np.float64).reshape(-1)
    se = np.sqrt(np.diag(V))
    stat = est / se
    return Frame({"name": list(names), "estimate": est, "se": se, "stat": stat,
                  "pvalue": np.array([pval(float(t)) for t in stat])})


# ---- one-way fixed effects (GLM.fit_fe): the array logic, no device ----
def fe_codes(labels):
    """(unique labels, dense codes) of a factor of any dtype (np.unique)."""
    uniq, codes = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    return uniq, codes.reshape(-1).astype(np.int64)


def fe_drop_intercept(X, names):
    """X without its intercept columns (every entry exactly 1): the fixed effects absorb the intercept."""
    X = np.asarray(X, dtype=np.float64)
    keep = [j for j in range(X.shape[1]) if not (X.shape[0] > 0 and np.all(X[:, j] == 1.0))]
    return np.asfortranarray(X[:, keep]), [names[j] for j in keep]


def fe_uninformative(codes, G, y, family, m=None, prior=None):
    """Mask [G] of the groups without a finite fixed effect: the rows of positive prior weight all have
    y = 0 (poisson, negbin, binomial) or all y = m (binomial).  A group with no such row is not one."""
    if family not in ("binomial", "poisson", "negbin"):
        return np.zeros(G, dtype=bool)
    y = np.asarray(y, dtype=np.float64)
    pos = np.ones(len(y), dtype=bool) if prior is None else np.asarray(prior) > 0
    a = np.bincount(codes[pos], weights=y[pos], minlength=G)
    other = (np.ones(len(y)) if m is None else np.asarray(m, dtype=np.float64)) - y if family == "binomial" \
        else np.ones(len(y))
    b = np.bincount(codes[pos], weights=other[pos], minlength=G)
    return (a == 0) != (b == 0)


def fe2_drop(codes1, codes2, y, family, m=None, prior=None):
    """(keep [n] bool, rounds): the rows left after the levels without a finite effect are dropped from either
    factor again and again until none is left -- dropping a unit's rows can leave a period with only zeros."""
    n = len(y)
    keep = np.ones(n, dtype=bool)
    rounds = 0
    c1, c2 = np.asarray(codes1).reshape(-1), np.asarray(codes2).reshape(-1)
    G, H = (int(c1.max()) + 1, int(c2.max()) + 1) if n else (0, 0)
    pr = np.ones(n) if prior is None else np.asarray(prior, dtype=np.float64)
    while True:
        w = np.where(keep, pr, 0.0)  # a dropped row counts as a row without weight
        bad = fe_uninformative(c1, G, y, family, m, w)[c1] | fe_uninformative(c2, H, y, family, m, w)[c2]
        bad &= keep
        if not bad.any():
            return keep, rounds
        keep &= ~bad
        rounds += 1


def fe_offsets(fixef, labels, offset=None):
    """offset + alpha[label] per row; NaN where the label is not among the fitted effects."""
    labels = np.asarray(labels).reshape(-1)
    a = np.array([fixef.get(l.item() if hasattr(l, "item") else l, np.nan) for l in labels], dtype=np.float64)
    return a if offset is None else a + np.asarray(offset, dtype=np.float64)


@dataclass
class FeData:
    """The arrays of a fixed-effects fit: the engine's family and link, X without its intercept and the names of
    its columns, the row vectors (None: not given), the labels and dense codes of the factor (of both factors of
    a two-way fit) and what was dropped as uninformative: levels over both factors, and rows."""
    fam: str
    lnk: str
    X: np.ndarray
    names: List[str]
    y: np.ndarray
    m: Optional[np.ndarray]
    offset: Optional[np.ndarray]
    prior: Optional[np.ndarray]
    labels: np.ndarray
    codes: np.ndarray
    labels2: Optional[np.ndarray] = None
    codes2: Optional[np.ndarray] = None
    dropped: int = 0
    dropped_rows: int = 0

    def drop(self, keep, nlev: int, quiet: bool):
        """Only the rows of `keep` stay, the factors are coded again; nlev levels go with the other rows."""
        self.dropped, self.dropped_rows = nlev, int((~keep).sum())
        if not quiet:
            print(f"NOTE: {nlev} fixed effect(s) ({self.dropped_rows} rows) removed because of only 0"
                  f"{' (or only m)' if self.fam == 'binomial' else ''} outcomes.")
        self.X, self.y = np.asfortranarray(self.X[keep]), self.y[keep]
        self.m, self.offset, self.prior = (None if v is None else v[keep] for v in (self.m, self.offset, self.prior))
        self.labels, self.codes = fe_codes(self.labels[self.codes[keep]])
        if self.codes2 is not None:
            self.labels2, self.codes2 = fe_codes(self.labels2[self.codes2[keep]])

    def load(self, theta, device: int) -> Engine:
        """The data and the factors on the device's engine."""
        eng = _engine(device)
        if self.fam == "negbin":
            _require(theta is not None, "family negbin needs theta (GLM.fit_nb estimates it without fixed effects)")
            eng.set_theta(theta)
        eng.set_data(self.X, self.y, self.m, self.offset, self.prior)
        eng.set_clusters(self.codes, len(self.labels))
        if self.codes2 is not None:
            eng.set_fe2(self.codes2, len(self.labels2))
        return eng


class GLM:
    """Namespace mirroring `object GLM` (GLM.scala:55-1026)."""

    @staticmethod
    def createObj(x: Frame, y: Frame, pre: PreGLM, family: str, link: str) -> GLMModel:
        """GLM.scala:59-88 (derived fields computed by sglm_glm_create_obj)."""
        lib = L.load()
        s, keep = _pre_struct(pre)
        s.nrow = float(y.count())
        d = L.GlmDerived()
        L.check(lib.sglm_glm_create_obj(C.byref(s), len(pre.stdErr), C.byref(d)))
        return GLMModel(x.columns, y.columns[0], pre.coefs, pre.stdErr, d.df_residual, d.df_null, pre.deviance,
                        pre.nullDeviance, d.p_dispersion, pre.pearson, pre.loglik, family, link, d.aic, pre.iter,
                        pre.nrow, pre.npart)

    @staticmethod
    def fit(y: Frame, x: Frame, *args, device: int = 0) -> GLMModel:
        """The sixteen Scala overloads (GLM.scala:597-995), dispatched on argument types."""
        args = list(args)
        offset = None
        if args and isinstance(args[0], Frame):
            offset = args.pop(0)
        _require(len(args) >= 2 and isinstance(args[0], str) and isinstance(args[1], str),
                 "fit(y, x, [offset,] family, link, ...)")
        family, link = args[0], args[1]
        tol, m, verbose = 1e-6, None, False
        rest = args[2:]
        kinds = []
        for a in rest:
            if isinstance(a, bool):
                verbose = a
                kinds.append("verbose")
            elif isinstance(a, (float, int)):
                tol = float(a)
                kinds.append("tol")
            elif isinstance(a, Frame):
                m = a
                kinds.append("m")
            else:
                raise TypeError(f"unsupported overload argument {a!r}")
        _require(kinds in ([], ["m"], ["tol"], ["tol", "m"], ["verbose"], ["m", "verbose"], ["tol", "verbose"],
                           ["tol", "m", "verbose"]), "no GLM.fit overload matches the arguments")
        _check_inputs(y, x)
        npart = x.rdd.partitions.size()
        four_arg = offset is None and not kinds
        if strict:
            if offset is not None and kinds == ["tol", "m"]:
                offset = None  # GLM.scala:789-792: this overload calls fitSingle without the offset
            if npart > 1 and not four_arg:
                # "Will change to fitDouble": fitSingle -> dfToDenseMatrix requires one partition
                _single_partition(x)
        pre = _fit_components(y, x, family, link, tol, verbose, offset=offset, m=m, device=device)
        return GLM.createObj(x, y, pre, family, link)

    @staticmethod
    def fit_weighted(y: Frame, x: Frame, family: str, link: str, prior: Frame, offset: Frame = None,
                     m: Frame = None, tol: float = 1e-6, verbose: bool = False, device: int = 0) -> GLMModel:
        """Extension: prior weights (R's `weights=`), on any partitioning."""
        _check_inputs(y, x)
        global strict
        saved, strict = strict, False
        try:
            pre = _fit_components(y, x, family, link, tol, verbose, offset=offset, m=m, prior=prior, device=device)
        finally:
            strict = saved
        return GLM.createObj(x, y, pre, family, link)

    @staticmethod
    def fit_nb(y: Frame, x: Frame, link: str = "log", theta: Optional[float] = None, offset: Frame = None,
               prior: Frame = None, tol: float = 1e-6, maxit: int = 0, epsilon: float = 0.0, theta_limit: int = 0,
               theta_eps: float = 0.0, device: int = 0) -> GLMModel:
        """Extension: the negative binomial family, V = mu + mu^2 / theta, links "log" (default), "sqrt",
        "identity".  With `theta` it is R's glm(..., family = MASS::negative.binomial(theta)); with
        theta=None it is MASS::glm.nb: theta by maximum likelihood, alternating with the fit (`maxit`,
        `epsilon`: glm.control's of the alternation; `theta_limit`, `theta_eps`: theta.ml's; zeros take
        R's defaults 25 / 1e-8 / 25 / 2^-13).  The model carries `theta`, and for glm.nb `theta_se` and
        `twologlik`; vcov, vcov_cluster, coeftest, influence and predict work on it."""
        _check_inputs(y, x)
        _require(link in L.NEGBIN_LINKS, f"family negbin supports only the {', '.join(L.NEGBIN_LINKS)} links")
        npart = x.rdd.partitions.size()
        for extra in (offset, prior):
            if extra is not None:
                _require(extra.count() == y.count(), "The two DataFrames must have the same number of rows")
        eng = _engine(device)
        eng.set_data(x.to_matrix(), y.to_vector(), None, None if offset is None else offset.to_vector(),
                     None if prior is None else prior.to_vector())
        init = "single" if npart == 1 else "multiple"
        if theta is not None:
            eng.set_theta(theta)
            f, th, se, tll = eng.fit_glm("negbin", link, tol=tol, init=init, npart=npart), float(theta), None, None
        else:
            r = eng.fit_glm_nb(link, tol=tol, init=init, npart=npart, maxit=maxit, epsilon=epsilon,
                               theta_limit=theta_limit, theta_eps=theta_eps)
            f, th, se, tll = r.fit, r.theta, r.se_theta, r.twologlik
        obj = GLM.createObj(x, y, _to_pre(f), "negbin", link)
        obj.theta, obj.theta_se, obj.twologlik = th, se, tll
        if theta is None:
            obj.aic += 2.0  # theta was estimated: one more parameter (logLik.negbin's df)
        return obj

    @staticmethod
    def fit_firth(y: Frame, x: Frame, family: str = "binomial", link: str = "logit", offset: Frame = None,
                  m: Frame = None, prior: Frame = None, epsilon: float = 1e-8, maxit: int = 100,
                  device: int = 0) -> GLMModel:
        """Extension: Firth's bias-reduced (penalized-likelihood) fit -- logistf::logistf, brglm2::brglmFit(type =
        "AS_mean"), Stata firthlogit -- of binomial (logit, probit, cloglog) and poisson (log, identity, sqrt)
        models with at most 256 columns: finite coefficients under separation.  The model carries `pen_deviance`,
        `logdet`, `halvings`, `converged` (False after `maxit` steps) and aic = None; predict, GLM.vcov,
        GLM.vcov_cluster, GLM.influence and GLM.coeftest work on it unchanged."""
        fam = family.lower() if isinstance(family, str) else family
        _require(fam in L.FIRTH_LINKS, "GLM.fit_firth takes family binomial or poisson (no dispersion families)")
        _require(link in L.FIRTH_LINKS[fam], f"family {family} supports only the {', '.join(L.FIRTH_LINKS[fam])} links")
        _require(isinstance(epsilon, (int, float)) and np.isfinite(epsilon) and epsilon > 0,
                 "epsilon is finite and > 0")
        _require(isinstance(maxit, (int, np.integer)) and maxit >= 0, "maxit is an integer >= 0")
        _check_inputs(y, x)
        for extra in (offset, m, prior):
            if extra is not None:
                _require(extra.count() == y.count(), "The two DataFrames must have the same number of rows")
        npart = x.rdd.partitions.size()
        eng = _engine(device)
        eng.set_data(x.to_matrix(), y.to_vector(), None if m is None else m.to_vector(),
                     None if offset is None else offset.to_vector(), None if prior is None else prior.to_vector())
        r = eng.fit_glm_firth(fam, link, epsilon, maxit, init="single" if npart == 1 else "multiple", npart=npart)
        obj = GLM.createObj(x, y, _to_pre(r.fit), fam, link)
        obj.pen_deviance, obj.logdet, obj.halvings, obj.converged, obj.aic = (r.pen_deviance, r.logdet, r.halvings,
                                                                              r.converged, None)
        return obj

    @staticmethod
    def _gee_engine(y, x, cluster, fam, lnk, offset, m, prior, theta, device, xnames=None) -> Engine:
        _check_inputs(y, x)
        for extra in (offset, m, prior):
            if extra is not None:
                _require(extra.count() == y.count(), "The two DataFrames must have the same number of rows")
        eng = _engine(device)
        if fam == "negbin":
            _require(theta is not None, "family negbin needs theta")
            eng.set_theta(theta)
        eng.set_data((x if xnames is None else x.select(*xnames)).to_matrix(), y.to_vector(),
                     None if m is None else m.to_vector(), None if offset is None else offset.to_vector(),
                     None if prior is None else prior.to_vector())
        _set_clusters(eng, cluster, y.count())
        return eng

    @staticmethod
    def fit_gee(y: Frame, x: Frame, cluster: Frame, family: str = "poisson", link: str = "log",
                corstr: str = "exchangeable", rho: Optional[float] = None, offset: Frame = None, m: Frame = None,
                prior: Frame = None, tol: float = 1e-6, verbose: bool = False, theta: Optional[float] = None,
                device: int = 0) -> GLMModel:
        """Extension: the population-averaged fit by generalized estimating equations (Liang & Zeger;
        geepack::geeglm(id = cluster, corstr =), Stata xtgee, statsmodels GEE).  `cluster` holds one column of
        labels of any dtype; `corstr` "exchangeable" (rho estimated by moments, or fixed at `rho`) or
        "independence".  The model carries `rho`, `scale` (phi), `corstr`, stdErr = the robust standard errors
        (what those packages print), `naive_se` = sqrt(phi diag(inv(A))), and aic = None: there is no
        likelihood.  GLM.vcov_gee, coeftest(gee=), summary and predict work on it."""
        fam, lnk = ("negbin", link) if family.lower() == "negbin" else _engine_family_link(family, link)
        eng = GLM._gee_engine(y, x, cluster, fam, lnk, offset, m, prior, theta, device)
        r = eng.fit_glm_gee(fam, lnk, corstr=corstr, rho=rho, tol=tol, verbose=verbose)
        V = eng.vcov_gee(r.fit.coefs, r.rho, fam, lnk, corstr=corstr)
        obj = GLM.createObj(x, y, _to_pre(r.fit), family, link)
        obj.naive_se = list(np.sqrt(r.phi) * r.fit.stderr)
        obj.stdErr = list(np.sqrt(np.diag(V)))
        obj.corstr, obj.rho, obj.scale, obj.aic = corstr, r.rho, r.phi, None
        if fam == "negbin":
            obj.theta = float(theta)
        return obj

    @staticmethod
    def vcov_gee(obj: GLMModel, y: Frame, x: Frame, cluster: Frame, offset: Frame = None, m: Frame = None,
                 prior: Frame = None, device: int = 0, robust: bool = True, cadjust: bool = False) -> np.ndarray:
        """Extension: the covariance of a GLM.fit_gee model's coefficients on its estimation data at the
        model's rho: robust (the sandwich over the clusters; `cadjust` a further G / (G - 1)), or with
        robust=False the model-based phi inv(A).  Final either way."""
        _require(getattr(obj, "corstr", None) is not None, "GLM.vcov_gee takes a GLM.fit_gee model")
        fam, lnk = _model_family_link(obj)
        eng = GLM._gee_engine(y, x, cluster, fam, lnk, offset, m, prior, obj.theta, device, obj.xnames)
        beta = np.asarray(obj.coefs, dtype=np.float64).reshape(-1)
        return eng.vcov_gee(beta, obj.rho, fam, lnk, corstr=obj.corstr, robust=robust, cadjust=cadjust)

    @staticmethod
    def _fe_data(y, x, fe, family, link, offset, m, prior, drop_uninformative, quiet=False) -> FeData:
        """The arrays of a fixed-effects fit: the intercept removed, the labels coded, uninformative groups
        dropped."""
        _check_inputs(y, x)
        _require(len(fe.columns) == 1, "The 'fe' DataFrame must have only one column")
        n = y.count()
        for extra in (fe, offset, m, prior):
            if extra is not None:
                _require(extra.count() == n, "The two DataFrames must have the same number of rows")
        fam = family.lower()
        if fam == "negbin":
            _require(link in L.NEGBIN_LINKS, f"family negbin supports only the {', '.join(L.NEGBIN_LINKS)} links")
            lnk = link
        else:
            fam, lnk = _engine_family_link(family, link)
        X, names = fe_drop_intercept(x.to_matrix(), x.columns)
        _require(len(names) >= 1, "x holds no column beside the intercept, which the fixed effects absorb")
        vec = lambda f: None if f is None else f.to_vector()
        yv, mv, ov, pv = y.to_vector(), vec(m), vec(offset), vec(prior)
        labels, codes = fe_codes(fe[fe.columns[0]])
        d = FeData(fam, lnk, X, names, yv, mv, ov, pv, labels, codes)
        bad = fe_uninformative(codes, len(labels), yv, fam, mv, pv)
        if bad.any() and drop_uninformative:
            d.drop(~bad[codes], int(bad.sum()), quiet)
        return d

    @staticmethod
    def _fe2_data(y, x, fe, fe2, family, link, offset, m, prior, drop_uninformative, quiet=False) -> FeData:
        """The arrays of a two-way fit: _fe_data's with the second factor coded too and the uninformative levels
        of either factor dropped until none is left."""
        _require(len(fe2.columns) == 1, "The 'fe2' DataFrame must have only one column")
        _require(fe2.count() == y.count(), "The two DataFrames must have the same number of rows")
        d = GLM._fe_data(y, x, fe, family, link, offset, m, prior, False, quiet=True)
        d.labels2, d.codes2 = fe_codes(fe2[fe2.columns[0]])
        if drop_uninformative:
            keep, _ = fe2_drop(d.codes, d.codes2, d.y, d.fam, d.m, d.prior)
            if not keep.all():
                left = len(np.unique(d.codes[keep])) + len(np.unique(d.codes2[keep]))
                nlev = len(d.labels) + len(d.labels2) - left
                d.drop(keep, nlev, quiet)
        return d

    @staticmethod
    def fit_fe(y: Frame, x: Frame, fe: Frame, family: str = "poisson", link: str = "log", offset: Frame = None,
               m: Frame = None, prior: Frame = None, drop_uninformative: bool = True, tol: float = 1e-6,
               verbose: bool = False, theta: Optional[float] = None, device: int = 0, fe2: Frame = None,
               sweep_tol: float = 0.0, max_sweeps: int = 0) -> GLMModel:
        """Extension: the GLM with one fixed effect per level of `fe` (one column of labels of any dtype),
        absorbed rather than expanded into dummy columns (fixest::feglm / fepois, Stata's xtpoisson, fe):
        coefficients, standard errors, deviances and iterations are those of GLM.fit on [x | dummies of fe].
        An intercept column of `x` is removed (the effects absorb it); a column that is constant within
        every level raises MatrixSingularException.  Groups whose outcomes are all 0 (binomial: or all m)
        have no finite effect: they are dropped with a note, as fixest does (drop_uninformative=False: the
        engine refuses the fit).  The model carries `fixef` (label -> alpha), dfResidual = n - p - G_eff and
        the counts of dropped groups and rows; family "negbin" fits at the given `theta`.  For binomial
        models with few rows per level the estimates carry the incidental-parameters bias of every
        dummy-variable fit (the engine applies no correction).

        With `fe2` (one more column of labels of any dtype) the fit absorbs two factors (fixest's feglm with
        `| fe + fe2`; sglm_fit_glm_fe2): uninformative levels of either factor are dropped repeatedly until
        none is left, the model carries `fixef` and `fixef2` (gamma is 0 at the lowest label of every connected
        component of the levels), dfResidual = n - p - (G_eff + H_eff - components), and `sweep_tol` /
        `max_sweeps` bound the alternating sweeps (0: 1e-12 and 10000).  One device, no communicator."""
        two = fe2 is not None
        if two:
            d = GLM._fe2_data(y, x, fe, fe2, family, link, offset, m, prior, drop_uninformative)
        else:
            d = GLM._fe_data(y, x, fe, family, link, offset, m, prior, drop_uninformative)
        eng = d.load(theta, device)
        npart = x.rdd.partitions.size()
        kw = dict(tol=tol, verbose=verbose, init="single" if npart == 1 else "multiple", npart=npart)
        r = eng.fit_glm_fe2(d.fam, d.lnk, sweep_tol=sweep_tol, max_sweeps=max_sweeps, **kw) if two else \
            eng.fit_glm_fe(d.fam, d.lnk, **kw)
        obj = GLM.createObj(x.select(*d.names), y, _to_pre(r.fit), "negbin" if d.fam == "negbin" else family, link)
        neff = r.G_eff + r.H_eff - r.ncomp if two else r.G_eff
        obj.dfResidual, obj.dfNull = float(r.df_residual), float(r.fit.nrow - 1.0)
        obj.pDispersion = obj.pearson / obj.dfResidual
        obj.aic = -2.0 * obj.loglik + 2.0 * (len(d.names) + neff)  # createObj's rule with the effects counted
        obj.theta = None if d.fam != "negbin" else float(theta)
        item = lambda l: l.item() if hasattr(l, "item") else l
        obj.fixef = {item(l): float(a) for l, a in zip(d.labels, r.alpha)}
        obj.fe_dropped_groups, obj.fe_dropped_rows = d.dropped, d.dropped_rows
        if two:
            obj.fixef2 = {item(l): float(a) for l, a in zip(d.labels2, r.gamma)}
            obj.fe_ncomp, obj.fe_sweeps = r.ncomp, r.sweeps
        return obj

    @staticmethod
    def _load_fe(obj: GLMModel, y, x, fe, offset, m, prior, device, fe2=None):
        """The model's estimation data on the engine with its factor as clusters (a two-way model: both
        factors), and (beta, alpha, gamma) -- gamma None without fe2."""
        two = fe2 is not None
        xs = x.select(*obj.xnames)
        if two:
            _require(obj.fixef is not None and obj.fixef2 is not None, "fe2 belongs to a GLM.fit_fe(fe2=) model")
            d = GLM._fe2_data(y, xs, fe, fe2, obj.family, obj.link, offset, m, prior, True, quiet=True)
        else:
            _require(obj.fixef is not None, "fe belongs to a GLM.fit_fe model")
            d = GLM._fe_data(y, xs, fe, obj.family, obj.link, offset, m, prior, True, quiet=True)
        eng = d.load(obj.theta, device)
        known = all(l in obj.fixef for l in d.labels.tolist())
        if two:
            _require(known and all(l in obj.fixef2 for l in d.labels2.tolist()),
                     "fe / fe2 hold a label the model was not fitted with")
        else:
            _require(known, "fe holds a label the model was not fitted with")
        return (eng, d.fam, d.lnk, np.asarray(obj.coefs, dtype=np.float64).reshape(-1), fe_offsets(obj.fixef, d.labels),
                fe_offsets(obj.fixef2, d.labels2) if two else None)

    @staticmethod
    def _load(obj: GLMModel, y: Frame, x: Frame, offset, m, prior, device):
        _check_inputs(y, x)
        fam, lnk = _model_family_link(obj)
        eng = _engine(device)
        if fam == "negbin":
            eng.set_theta(obj.theta)
        eng.set_data(x.select(*obj.xnames).to_matrix(), y.to_vector(), None if m is None else m.to_vector(),
                     None if offset is None else offset.to_vector(), None if prior is None else prior.to_vector())
        return eng, fam, lnk, np.asarray(obj.coefs, dtype=np.float64).reshape(-1)

    @staticmethod
    def vcov(obj: GLMModel, y: Frame, x: Frame, offset: Frame = None, m: Frame = None, prior: Frame = None,
             device: int = 0, type: str = "const") -> np.ndarray:
        """Extension: the unscaled covariance inv(X'WX) at the fitted coefficients (R's
        summary(fit)$cov.unscaled); multiply by the dispersion for vcov(fit).  `type` "HC0".."HC3":
        the sandwich covariance (sandwich::vcovHC) instead, which is final -- no dispersion applies.
        (A GLM.fit_fe model: GLM.vcov_fe, which takes the factor.)"""
        _require(getattr(obj, "fixef", None) is None, "a fixed-effects model needs its factor: GLM.vcov_fe(obj, y, x, fe)")
        _check_cov_type(type)
        eng, fam, lnk, beta = GLM._load(obj, y, x, offset, m, prior, device)
        return eng.vcov(beta, fam, lnk) if type == "const" else eng.vcov_robust(beta, fam, lnk, type=type)

    @staticmethod
    def vcov_fe(obj: GLMModel, y: Frame, x: Frame, fe: Frame, offset: Frame = None, m: Frame = None,
                prior: Frame = None, device: int = 0, type: str = "const", cadjust: bool = True,
                fe2: Frame = None) -> np.ndarray:
        """Extension: the covariance of a GLM.fit_fe model's coefficients on its estimation data, `fe` its
        factor.  `type` "const": inv(A), the beta block of the dummy fit's unscaled covariance (multiply by
        the dispersion); "HC0" / "HC1": clustered on `fe` (sglm_vcov_fe), the beta block of
        sandwich::vcovCL on the dummy fit, `cadjust` as GLM.vcov_cluster -- final.  (GLM.vcov keeps its
        signature; a fixed-effects model is refused there.)"""
        if type != "const":
            _check_cluster_type(type)
        if fe2 is not None or getattr(obj, "fixef2", None) is not None:  # two-way: clustered on fe (factor 1)
            _require(fe2 is not None, "a two-way fixed-effects model needs fe2 as well")
            eng, fam, lnk, beta, alpha, gamma = GLM._load_fe(obj, y, x, fe, offset, m, prior, device, fe2)
            return eng.vcov_fe2(beta, alpha, gamma, fam, lnk, cluster=type != "const",
                                type=type if type != "const" else "HC0", cadjust=cadjust)
        eng, fam, lnk, beta, alpha, _ = GLM._load_fe(obj, y, x, fe, offset, m, prior, device)
        return eng.vcov_fe(beta, alpha, fam, lnk, cluster=type != "const", type=type if type != "const" else "HC0",
                           cadjust=cadjust)

    @staticmethod
    def vcov_cluster(obj: GLMModel, y: Frame, x: Frame, cluster: Frame, offset: Frame = None, m: Frame = None,
                     prior: Frame = None, device: int = 0, type: str = "HC1", cadjust: bool = True) -> np.ndarray:
        """Extension: the cluster-robust covariance sandwich::vcovCL(fit, cluster = ~id, type, cadjust)
        at the fitted coefficients; `cluster` holds one column of labels, one per row.  `type` "HC0" or
        "HC1"; the defaults are vcovCL's (and Stata's regress, vce(cluster)).  Final, as the sandwich."""
        _check_cluster_type(type)
        eng, fam, lnk, beta = GLM._load(obj, y, x, offset, m, prior, device)
        _set_clusters(eng, cluster, y.count())
        return eng.vcov_cluster(beta, fam, lnk, type=type, cadjust=cadjust)

    @staticmethod
    def coeftest(obj: GLMModel, y: Frame, x: Frame, offset: Frame = None, m: Frame = None, prior: Frame = None,
                 device: int = 0, type: str = "HC3", cluster: Frame = None, cadjust: bool = True,
                 fe: Frame = None, fe2: Frame = None, gee: Frame = None) -> Frame:
        """Extension: lmtest::coeftest(fit, vcov. = vcovHC(fit, type)) -- name, estimate, robust
        standard error sqrt(diag V), z statistic and its two-sided normal p-value.  With `cluster` (one
        column of labels) the covariance is vcovCL(fit, cluster, type, cadjust) and `type` must be "HC0"
        or "HC1".  A GLM.fit_fe model takes its factor `fe` and is clustered on it by default (`type` "HC1"
        unless "HC0" or "const" is given).  A GLM.fit_gee model takes its cluster frame `gee`: z statistics on
        the robust covariance (GLM.vcov_gee; `type` does not apply).  `cadjust` keeps this function's default, True
        (vcovCL's), so the table's standard errors are sqrt(G / (G - 1)) times the model's stdErr, which
        GLM.fit_gee and GLM.vcov_gee form without it as geepack and statsmodels do; cadjust=False gives stdErr."""
        if gee is not None or getattr(obj, "corstr", None) is not None:
            _require(gee is not None and getattr(obj, "corstr", None) is not None,
                     "gee belongs to a GLM.fit_gee model, which needs it")
            _require(cluster is None and fe is None, "a GEE model is clustered on its own factor gee")
            V = GLM.vcov_gee(obj, y, x, gee, offset, m, prior, device, True, cadjust)
            beta = np.asarray(obj.coefs, dtype=np.float64).reshape(-1)
            return _coef_table(obj.xnames, beta, V, L.load().sglm_pval_normal)
        if fe is not None or getattr(obj, "fixef", None) is not None:
            _require(cluster is None, "a fixed-effects model is clustered on its own factor fe")
            t = type if type in ("const", "HC0", "HC1") else "HC1"
            _require(fe is not None and getattr(obj, "fixef", None) is not None, "fe belongs to a GLM.fit_fe model, which needs it")
            V = GLM.vcov_fe(obj, y, x, fe, offset, m, prior, device, t, cadjust, fe2=fe2)
            beta = np.asarray(obj.coefs, dtype=np.float64).reshape(-1)
            return _coef_table(obj.xnames, beta, V, L.load().sglm_pval_normal)
        if cluster is not None:
            V = GLM.vcov_cluster(obj, y, x, cluster, offset, m, prior, device, type, cadjust)
            beta = np.asarray(obj.coefs, dtype=np.float64).reshape(-1)
            return _coef_table(obj.xnames, beta, V, L.load().sglm_pval_normal)
        if type not in L.HC_TYPES:
            raise L.IllegalArgumentException(f"requirement failed: type must be one of {sorted(L.HC_TYPES)}, "
                                             f"got {type!r}")
        eng, fam, lnk, beta = GLM._load(obj, y, x, offset, m, prior, device)
        return _coef_table(obj.xnames, beta, eng.vcov_robust(beta, fam, lnk, type=type), L.load().sglm_pval_normal)

    @staticmethod
    def influence(obj: GLMModel, y: Frame, x: Frame, offset: Frame = None, m: Frame = None, prior: Frame = None,
                  type: str = "deviance", device: int = 0):
        """Extension: R's hatvalues / residuals(type=) / cooks.distance of the fitted model on its
        estimation data, as an engine.Influence.  The dispersion of Cook's distance is 1 for binomial
        and poisson and obj.pDispersion for gaussian and gamma (R's rule).  Binomial residuals are on
        the count scale (divide by m for R's proportion scale)."""
        if type not in L.RESID_TYPES:
            raise L.IllegalArgumentException(f"requirement failed: type must be one of {sorted(L.RESID_TYPES)}, "
                                             f"got {type!r}")
        eng, fam, lnk, beta = GLM._load(obj, y, x, offset, m, prior, device)
        return eng.influence(beta, fam, lnk, resid=type, dispersion=_dispersion(obj))

    @staticmethod
    def summary_string(obj: GLMModel) -> str:
        lib = L.load()
        pre = PreGLM(obj.coefs, obj.stdErr, obj.deviance, obj.nullDeviance, obj.pearson, obj.loglik, obj.iter,
                     obj.nrow, obj.npart)
        s, keep = _pre_struct(pre)
        names = (C.c_char_p * len(obj.xnames))(*[n.encode() for n in obj.xnames])
        need = lib.sglm_glm_summary(C.byref(s), len(obj.xnames), names, obj.yname.encode(), obj.family.encode(),
                                    obj.link.encode(), None, 0)
        buf = C.create_string_buffer(int(need))
        lib.sglm_glm_summary(C.byref(s), len(obj.xnames), names, obj.yname.encode(), obj.family.encode(),
                             obj.link.encode(), buf, need)
        text = buf.value.decode()
        if getattr(obj, "corstr", None) is not None:  # GLM.fit_gee: no likelihood, the correlation and the scale
            text = _gee_summary(text, obj, lib)
        elif getattr(obj, "pen_deviance", None) is not None:  # GLM.fit_firth
            text = _firth_summary(text, obj, lib)
        elif getattr(obj, "theta", None) is not None:  # GLM.fit_nb: theta, and the AIC that counts it when estimated
            text = _nb_summary(text, obj, lib)
        return text

    @staticmethod
    def summary(obj: GLMModel) -> None:
        """GLM.scala:998-1025 (prints)."""
        print(GLM.summary_string(obj), end="")
