"""Multinomial logit fits (softmax regression) over Frames: nnet::multinom, Stata's mlogit, statsmodels' MNLogit.

`Multinom.fit(y, x, prior=None)` codes the labels of y (any dtype; the levels sorted, the first the baseline), runs
sglm_fit_multinom on the GPU and returns a MultinomModel with the named (K - 1) x p tables.  New rows are scored
through the engine's sglm_predict_new, one call per class, with the softmax on the host.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib as L
from .frame import Frame
from .glm import _engine, _require


def code_levels(labels):
    """(levels sorted, codes as float64 in 0 .. K - 1): the first level is the baseline."""
    levels, codes = np.unique(np.asarray(labels), return_inverse=True)
    return levels, codes.astype(np.float64).reshape(-1)


def softmax_link(eta):
    """[n, K] probabilities from the K - 1 linear predictors eta [n, K - 1] (class 0: eta = 0), formed against the
    row maximum."""
    e = np.c_[np.zeros(eta.shape[0]), eta]
    e = np.exp(e - np.max(e, axis=1, keepdims=True))
    return e / np.sum(e, axis=1, keepdims=True)


@dataclass
class MultinomModel:
    levels: np.ndarray       # K labels, sorted; levels[0] is the baseline
    xnames: List[str]
    yname: str
    coefs: np.ndarray        # [K - 1, p]: row j - 1 is levels[j] against the baseline
    stdErr: np.ndarray       # [K - 1, p]
    z: np.ndarray            # Wald z = coefs / stdErr
    pvalue: np.ndarray       # 2 (1 - Phi(|z|))
    cov: np.ndarray          # [q, q] over the class-major parameter vector
    deviance: float
    null_deviance: float
    loglik: float
    aic: float
    iter: int
    halvings: int
    converged: bool
    nrow: float              # the sum of the prior weights

    def table(self, what: str = "coefs") -> Frame:
        """One of coefs / stdErr / z / pvalue as a Frame: a `level` column, then a column per predictor."""
        v = getattr(self, what)
        cols = {"level": np.asarray(self.levels[1:])}
        cols.update({nm: v[:, j].copy() for j, nm in enumerate(self.xnames)})
        return Frame(cols)

    def predict(self, newData: Frame, type: str = "probs", device: int = 0):
        """"probs": [n, K] probabilities (columns in the order of `levels`); "class": the most probable level of
        each row; "link": [n, K - 1] linear predictors against the baseline."""
        _require(type in ("probs", "class", "link"), 'type is one of "probs", "class", "link"')
        _require(len(set(self.xnames) - set(newData.columns)) == 0,
                 "Not all predictors in the estimation data are in the data to be predicted")
        newX = newData.select(*self.xnames).to_matrix()
        eng = _engine(device)
        eta = np.column_stack([eng.predict_new(newX, np.ascontiguousarray(b), "gaussian", "identity", "link")
                               for b in self.coefs])
        if type == "link":
            return eta
        pr = softmax_link(eta)
        return pr if type == "probs" else np.asarray(self.levels)[np.argmax(pr, axis=1)]


class Multinom:
    @staticmethod
    def fit(y: Frame, x: Frame, prior: Optional[Frame] = None, epsilon: float = 1e-8, max_iter: int = 100,
            max_halvings: int = 12, device: int = 0) -> MultinomModel:
        _require(len(y.columns) == 1, "y has one column of class labels")
        _require(y.count() == x.count(), "The two DataFrames must have the same number of rows")
        _require(isinstance(epsilon, (int, float)) and not isinstance(epsilon, bool) and math.isfinite(epsilon)
                 and epsilon > 0, "epsilon is finite and > 0")
        _require(isinstance(max_iter, int) and max_iter >= 0, "max_iter is an integer >= 0")
        _require(isinstance(max_halvings, int) and max_halvings >= 0, "max_halvings is an integer >= 0")
        pw = None
        if prior is not None:
            _require(prior.count() == y.count(), "The two DataFrames must have the same number of rows")
            pw = prior.to_vector()
        levels, codes = code_levels(y[y.columns[0]])
        K, p = len(levels), len(x.columns)
        _require(2 <= K <= L.MULTINOM_MAX_K, f"2 <= the number of classes <= {L.MULTINOM_MAX_K} (got {K})")
        _require((K - 1) * p <= L.MULTINOM_MAX_Q,
                 f"(n_classes - 1) * p <= {L.MULTINOM_MAX_Q} (got {(K - 1) * p})")
        eng = _engine(device)
        eng.set_data(x.to_matrix(), codes, prior=pw)
        f = eng.fit_multinom(K, epsilon, max_iter, max_halvings=max_halvings)
        with np.errstate(all="ignore"):
            z = f.coefs / f.stderr
        lib = L.load()
        pv = np.array([lib.sglm_pval_normal(float(v)) for v in z.reshape(-1)]).reshape(z.shape)
        return MultinomModel(levels, list(x.columns), y.columns[0], f.coefs, f.stderr, z, pv, f.cov, f.deviance,
                             f.null_deviance, f.loglik, f.aic, f.iter, f.halvings, f.converged,
                             float(np.sum(f.class_weight)))

    @staticmethod
    def summary_string(obj: MultinomModel) -> str:
        lib = L.load()

        def sig(v):
            buf = C.create_string_buffer(64)
            lib.sglm_java_double_string(lib.sglm_sig_digits(float(v), 5), buf, 64)
            return buf.value.decode()

        q = obj.coefs.size
        out = ["Multinomial logit  " + obj.yname + " ~ " + " + ".join(obj.xnames),
               "Baseline: " + str(obj.levels[0]), ""]
        for j, lev in enumerate(obj.levels[1:]):
            out.append(f"{lev}:")
            out.append("\t".join(["", "Estimate", "Std. Error", "z value", "Pr(>|z|)"]))
            for c, nm in enumerate(obj.xnames):
                out.append("\t".join([nm] + [sig(t[j, c]) for t in (obj.coefs, obj.stdErr, obj.z, obj.pvalue)]))
            out.append("")
        out.append(f"Null Deviance: {sig(obj.null_deviance)} on {sig(obj.nrow)} weighted rows")
        out.append(f"Residual Deviance: {sig(obj.deviance)} with {q} parameters")
        out.append(f"Log-likelihood: {sig(obj.loglik)}    AIC: {sig(obj.aic)}")
        out.append(f"Number of Newton iterations: {obj.iter}" + ("" if obj.converged else " (not converged)"))
        return "\n".join(out) + "\n"

    @staticmethod
    def summary(obj: MultinomModel) -> None:
        print(Multinom.summary_string(obj), end="")
