"""The exact per-row functions of the IRLS pass (sparkglm_amd/csrc/rowmath.hpp), in np.longdouble.

TEST INFRASTRUCTURE ONLY (a helper module of tests/test_rowmath_reference.py and tests/test_gpu_rowmath.py).

exact(family, link, eta, y, m, off, pw, theta) gives, for fp64 inputs, the mathematical value of every
quantity a pass row produces -- the working weight w, w*z, the unit deviance (before the family factor) and,
for the pairs with in-pass statistics (logit, poisson/log, gamma/inverse), the Pearson term and the
log-likelihood terms of StatsSlots -- with, for each quantity q, its scale S_q and the row's amplification
kappa.  Errors are measured everywhere as

    err(q) = |got - exact| / (2^-53 * S_q)          ("eps units")

S_q is the sum of the magnitudes of the operands of the last additive step of the form rowmath.hpp documents
for q (nested differences of rounded operands flattened): what a correctly rounded evaluation of that form
is good to, whichever way the operands cancel.  kappa = 1 / min(mu/m, 1 - mu/m) for the binomial links -- the
reference operation order forms 1 - mu/m by subtraction, which loses that factor -- and 1 elsewhere.

The forms avoid cancellation: 1 - mu as e/(1+e), log1p on the small side, Phi's tails through erfc, the logs of
quotients formed in long double.  numpy has no long double erfc / lgamma: those two come from mpmath at 30 digits,
element by element, rounded to long double (a hi + lo pair of doubles); everything else is long double
arithmetic.  test_rowmath_reference.py checks the whole module against the textbook formulas in mpmath.

ref_order(...) restates pass_row_ref's operation order in fp64 numpy (the oracle's order; it is also where
the order runs to NaN), for the pairs the C oracle does not know (sqrt links, the negative binomial) and for
the grids' own conditions.  The fast-path gates are restated by fast_row(), compared in fp64 as the macros do.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended type: no reference finer than fp64 here"
EPS = 2.0 ** -53

BINOMIAL_LINKS = ("logit", "probit", "cloglog")
PAIRS = ([("binomial", l) for l in BINOMIAL_LINKS] +
         [("gaussian", l) for l in ("identity", "log", "inverse")] +
         [("poisson", l) for l in ("log", "identity", "sqrt")] +
         [("gamma", l) for l in ("inverse", "identity", "log")] +
         [("negbin", l) for l in ("log", "sqrt", "identity")])
STATS_PAIRS = (("binomial", "logit"), ("poisson", "log"), ("gamma", "inverse"))


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def to_mpf(v):
    """A long double as an mpf, exactly (mantissa as a hi + lo pair of doubles, then the exponent)."""
    import mpmath
    if not np.isfinite(v):
        return mpmath.mpf(float(v))
    mant, e = np.frexp(LD(v))
    hi = float(mant)
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(float(mant - LD(hi))), int(e))


def from_mpf(r):
    """An mpf rounded to long double (to within 2^-105 relative)."""
    import mpmath
    if r == 0 or not mpmath.isfinite(r):
        return LD(float(r))
    mant, e = mpmath.frexp(r)
    hi = float(mant)
    return np.ldexp(LD(hi) + LD(float(mant - mpmath.mpf(hi))), int(e))


def _via_mp(f, x, dps=30):
    """f (an mpmath function of one mpf) at every element of the long double array x, rounded to long double."""
    import mpmath
    out = np.empty(x.shape, dtype=LD)
    with mpmath.workdps(dps):
        for i, v in np.ndenumerate(x):
            out[i] = from_mpf(f(to_mpf(v)))
    return out


def _norm_tail(x):
    """Phi(x) = erfc(-x / sqrt 2) / 2: relatively accurate in both tails."""
    import mpmath
    return _via_mp(lambda t: mpmath.erfc(-t / mpmath.sqrt(2)) / 2, x)


def lgamma1p(y):
    """lgamma(y + 1) (the per-fit constant of the Poisson log-likelihood, init_stats_const)."""
    import mpmath
    return _via_mp(lambda t: mpmath.loggamma(t + 1), ld(y), dps=350)   # (y + 1 exact down to denormal y)


def _softplus(x):
    """log(1 + exp(x)) as max(x, 0) + log1p(exp(-|x|)): two non-negative terms."""
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _binomial_link(link, eta):
    """pi, q = 1 - pi, d = dpi/deta, log pi, log q of a binomial link at eta (long double)."""
    if link == "logit":
        a = np.exp(-np.abs(eta))                     # in (0, 1]
        big, small = 1 / (1 + a), a / (1 + a)
        pi = np.where(eta >= 0, big, small)
        q = np.where(eta >= 0, small, big)
        return pi, q, pi * q, -_softplus(-eta), -_softplus(eta)
    if link == "probit":
        pi, q = _norm_tail(eta), _norm_tail(-eta)
        d = np.exp(-eta * eta / 2) / np.sqrt(8 * np.arctan(LD(1)))
    else:  # cloglog
        ee = np.exp(eta)
        q = np.exp(-ee)
        pi = -np.expm1(-ee)
        d = ee * q
    with np.errstate(divide="ignore", invalid="ignore"):
        logpi = np.where(pi < 0.5, np.log(pi), np.log1p(-q))
        logq = np.where(q < 0.5, np.log(q), np.log1p(-pi))
    if link == "cloglog":
        logq = -ee
    return pi, q, d, logpi, logq


def _ext_link(link, eta):
    """mu and dmu/deta of R's make.link links."""
    if link == "identity":
        return eta, np.ones_like(eta)
    if link == "log":
        mu = np.exp(eta)
        return mu, mu
    if link == "inverse":
        return 1 / eta, -1 / (eta * eta)
    if link == "sqrt":
        return eta * eta, 2 * eta
    raise ValueError(link)


def _xlogx_ratio(y, ratio):
    """y log(ratio), 0 where y == 0 (the families' y log(y / mu) terms; the quotient is formed in long double, so
    that nothing cancels between two logs)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(y == 0, LD(0), y * np.log(ratio))


def exact(family, link, eta, y, m=None, off=None, pw=None, theta=None):
    """dict q -> (value, S_q) for q in w, wz, dev (and pearson, ll / aux0 / aux1 for STATS_PAIRS), plus
    "kappa", all long double arrays; inputs are the fp64 values the row sees (eta as the kernel rounded it)."""
    eta, y = ld(eta), ld(y)
    n = eta.shape
    has_m = m is not None
    m = np.ones(n, dtype=LD) if m is None else ld(m)
    off = np.zeros(n, dtype=LD) if off is None else ld(off)
    pw = np.ones(n, dtype=LD) if pw is None else ld(pw)
    out = {}
    with np.errstate(all="ignore"):
        if family == "binomial":
            pi, q, dpi, logpi, logq = _binomial_link(link, eta)
            mu, d, v = m * pi, m * dpi, m * pi * q
            kappa = 1 / np.minimum(pi, q)
            my = m - y
            ty = _xlogx_ratio(y, np.maximum(y, 1) / m) - y * logpi
            tm = _xlogx_ratio(my, np.maximum(my, 1) / m) - my * logq
            dev = pw * (ty + tm)
            inside = (y >= 0) & (y <= 1) if (link == "logit" and not has_m) else np.zeros(n, dtype=bool)
            # logit, m = 1, 0 <= y <= 1: log1p(e) + (1 - y) eta, e = exp(-eta)
            # other rows: the two terms of devBinomial, each with its factor itself beside it (the log's argument
            # is a rounded quotient: one unit of absolute error in the log, whatever the log's size)
            s_dev = np.where(inside, pw * (np.abs(_softplus(-eta)) + np.abs((1 - y) * eta)),
                             pw * (np.abs(ty) + np.abs(y) + np.abs(tm) + np.abs(my)))
        else:
            mu, d = _ext_link(link, eta)
            kappa = np.ones(n, dtype=LD)
            if family == "gaussian":
                v = np.ones(n, dtype=LD)
                dev, s_dev = pw * (y - mu) ** 2, pw * (np.abs(y) + np.abs(mu)) ** 2
            elif family == "poisson":
                v = mu
                t = _xlogx_ratio(y, y / mu)
                dev, s_dev = pw * (t - (y - mu)), pw * (np.abs(t) + np.abs(y) + np.abs(mu))
            elif family == "gamma":
                v = mu * mu
                lr = np.log(y / mu)
                dev, s_dev = pw * (-(lr - (y / mu - 1))), pw * (np.abs(lr) + np.abs(y / mu) + 1)
            elif family == "negbin":
                th = ld(np.broadcast_to(theta, n))
                v = mu + mu * mu / th
                t1 = _xlogx_ratio(y, np.maximum(y, 1) / mu)
                t2 = (y + th) * np.log((y + th) / (mu + th))
                # (y + theta beside its term: the log's argument is a rounded quotient or product, one unit of
                # absolute error in the log -- the Poisson scale's |y| + |mu| and the gamma scale's 1 are the same)
                dev, s_dev = pw * (t1 - t2), pw * (np.abs(t1) + np.abs(t2) + (y + th))
            else:
                raise ValueError(family)
        w = pw * d * d / v
        wg = pw * d / v                                  # w g'
        out["w"] = (w, np.abs(w))
        out["wz"] = (w * (eta - off) + wg * (y - mu), np.abs(w * (eta - off)) + np.abs(wg) * (np.abs(y) + np.abs(mu)))
        out["dev"] = (dev, s_dev)
        out["kappa"] = kappa
        if (family, link) in STATS_PAIRS:
            out["pearson"] = (pw * (y - mu) ** 2 / v, pw * (np.abs(y) + np.abs(mu)) ** 2 / np.abs(v))
        if (family, link) == ("binomial", "logit"):
            # Breeze Binomial(1, mu).logProbabilityOf(k), k = (int) y: k log mu + (1 - k) log(1 - mu), as
            # -L (k = 1) or -L - eta (k = 0) with L = log1p(exp(-eta)); rows with m: Binomial(m, mu / m)
            k = np.trunc(y)
            L = _softplus(-eta)
            out["ll"] = (pw * np.where(k == 1, logpi, logq), pw * np.where(k == 1, np.abs(L), np.abs(L) + np.abs(eta)))
        elif (family, link) == ("poisson", "log"):
            # S_LL without the per-fit constant sum pw lgamma(y + 1) (init_stats_const: the initial pass's S_AUX2)
            out["ll"] = (pw * (y * eta - mu), pw * (np.abs(y * eta) + np.abs(mu)))
            # R's dpois in full, as stats_row_ref sums it: y log mu - mu - lgamma(y + 1) (|y| beside y log mu: the
            # log's argument mu is a rounded exp; 1 beside lgamma: its argument y + 1 is a rounded sum)
            lg = lgamma1p(y)
            out["ll_full"] = (pw * (y * eta - mu - lg), pw * (np.abs(y * eta) + np.abs(y) + np.abs(mu) + np.abs(lg) + 1))
        elif (family, link) == ("gamma", "inverse"):
            # S_AUX0 = pw y / mu = pw y eta; the pass's S_AUX1 slot = pw log(y eta) (the host forms sum pw log mu
            # from it and the initial pass's sum pw log y)
            out["aux0"] = (pw * y * eta, np.abs(pw * y * eta))
            # (+ 1: the log's argument y eta is a rounded product, one unit of absolute error in the log)
            out["aux1"] = (pw * np.log(y * eta), pw * (np.abs(np.log(y * eta)) + 1))
            # the slots of the final statistics (ext_loglik_terms): sum pw log y and sum pw log mu (+ 1: mu = 1 / eta
            # is a rounded quotient)
            out["logy"] = (pw * np.log(y), pw * np.abs(np.log(y)))
            out["logmu"] = (-pw * np.log(eta), pw * (np.abs(np.log(eta)) + 1))
    return out


TINY = LD(2.0) ** -1074   # fp64's smallest quantum: a result below the normal range is held to it, not to eps S_q


def signed_units(got, value, scale):
    """(got - exact) / (2^-53 S_q + 2^-1074) per element; 0 where both are exactly equal (S_q = 0 included)."""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    with np.errstate(all="ignore"):
        e = (got - value) / (LD(EPS) * scale + TINY)
    return np.where(got == value, LD(0), e).astype(np.float64)


def units(got, value, scale):
    """|got - exact| / (2^-53 S_q + 2^-1074): the error in eps units."""
    return np.abs(signed_units(got, value, scale))


# ---- the gates of the fast paths, compared in fp64 exactly as rowmath.hpp's conditions do ----
def fast_row(family, link, eta, y, has_m=False, theta=None):
    eta, y = np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if (family, link) == ("binomial", "logit"):
        return (np.abs(eta) < 8.0) & (y >= 0.0) & (y <= 1.0) & (not has_m)
    if (family, link) == ("poisson", "log"):
        return (np.abs(eta) < 700.0) & (y >= 0.0) & (y < 1e300)
    if (family, link) == ("gamma", "inverse"):
        return (eta > 1e-150) & (eta < 1e150) & (y > 1e-150) & (y < 1e150)
    if (family, link) == ("gamma", "log"):
        return (np.abs(eta) < 300.0) & (y > 1e-150) & (y < 1e150)
    if (family, link) == ("negbin", "log"):
        th = np.broadcast_to(np.asarray(theta, dtype=np.float64), eta.shape)
        return (np.abs(eta) < 300.0) & (y >= 0.0) & (y < 1e150) & (th > 1e-150) & (th < 1e150)
    return np.zeros(eta.shape, dtype=bool)


FAST_PAIRS = (("binomial", "logit"), ("poisson", "log"), ("gamma", "inverse"), ("gamma", "log"), ("negbin", "log"))


# ---- pass_row_ref's operation order in fp64 (IRLS mode) ----
def _norm_cdf64(x):
    from scipy import special
    return 0.5 * (1.0 + special.erf(x / np.sqrt(2.0)))


def _norm_icdf64(q):
    from scipy import special
    return 0.0 + 1.0 * np.sqrt(2.0) * special.erfinv(2.0 * q - 1.0)


def _norm_pdf64(x):
    d = (x - 0.0) / 1.0
    return np.exp(-d * d / 2.0 - (np.log(np.sqrt(2.0 * np.pi)) + np.log(1.0)))


def ref_order(family, link, eta, y, m=None, off=None, pw=None, theta=None):
    """(w, wz, dev) of row_core / working_wz / unit_dev (rowmath.hpp) in fp64, operation for operation; a row
    outside its pair's validity (link_row_valid) carries a NaN unit deviance."""
    eta, y = np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = eta.shape
    m = np.ones(n) if m is None else np.asarray(m, dtype=np.float64)
    off = np.zeros(n) if off is None else np.asarray(off, dtype=np.float64)
    pw = np.ones(n) if pw is None else np.asarray(pw, dtype=np.float64)
    by_link = family == "negbin" or (family, link) in (("gaussian", "log"), ("gaussian", "inverse"), ("poisson", "identity"),
                                                        ("poisson", "sqrt"), ("gamma", "identity"), ("gamma", "log"))
    with np.errstate(all="ignore"):
        if family == "binomial":
            if link == "logit":
                mu = m / (1.0 + np.exp(-1.0 * eta))
                g = m / (mu * (m + (-1.0 * mu)))
            elif link == "probit":
                mu = m * _norm_cdf64(eta)
                g = 1.0 / (m * _norm_pdf64(_norm_icdf64(mu / m)))
            else:
                mu = m * (1.0 + (-1.0 * np.exp(-np.exp(eta))))
                g = 1.0 / ((mu + (-1.0 * m)) * np.log(1.0 + (-1.0 * (mu / m))))
            v = mu * (1.0 + (-1.0 * (mu / m)))
        else:
            lnk = link if by_link else {"gaussian": "identity", "poisson": "log", "gamma": "inverse"}[family]
            if lnk == "identity":
                mu, g = eta, np.ones(n)
            elif lnk == "log":
                mu = np.exp(eta)
                g = 1.0 / mu
            elif lnk == "inverse":
                mu = 1.0 / eta
                g = -1.0 / (mu * mu)
            else:
                mu = eta * eta
                g = 0.5 / np.sqrt(mu)
            if family == "gaussian":
                v = np.ones(n)
            elif family == "poisson":
                v = mu
            elif family == "gamma":
                v = mu * mu
            else:
                v = mu + (mu * mu) / theta
        w = pw * (1.0 / (v * (g * g)))
        z = (eta + ((y + (-1.0 * mu)) * g)) + (-1.0 * off)
        wz = w * z
        if family == "binomial":
            my = m + (-1.0 * y)
            dev = pw * ((y * np.log(np.maximum(y, 1.0) / mu)) + (my * np.log(np.maximum(my, 1.0) / (m + (-1.0 * mu)))))
        elif family == "gaussian":
            dev = pw * ((y - mu) * (y - mu))
        elif family == "poisson":
            dev = pw * (np.where(y > 0.0, y * np.log(y / mu), 0.0) - (y - mu))
        elif family == "gamma":
            dev = pw * (-(np.log(y / mu) - (y - mu) / mu))
        else:
            dev = pw * ((y * np.log(np.maximum(y, 1.0) / mu)) - ((y + theta) * np.log((y + theta) / (mu + theta))))
        if by_link:
            if family == "gaussian":
                ok = np.isfinite(eta) & ~((lnk == "inverse") & (eta == 0.0))
            else:
                ok = np.isfinite(mu) & (mu > 0.0) & ~((lnk == "sqrt") & ~(eta > 0.0))
            dev = np.where(ok, dev, np.nan)
    return w, wz, dev


# ---- the grids of tests/test_gpu_rowmath.py (checked on the CPU by tests/test_rowmath_reference.py) ----
# A grid is a list of groups; a group is dict(name, kind, eta, y[, m, off, pw, theta]) with fp64 arrays:
#   kind "fast"      dense rows inside the fast path's range              (assertion A)
#        "ref"       dense rows on the reference operation order          (assertion B)
#        "edge-fast" / "edge-ref"   the edge list, row by row             (A / B, the deviance isolated per row)
#        "nonfinite" rows whose reference order is not finite             (pattern against the oracle's)
# eta is the value the kernel forms: x = eta - off is exact for every row here (grid_conditions checks it).
def _grp(name, kind, eta, y, **kw):
    eta, y = np.broadcast_arrays(np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64))
    g = dict(name=name, kind=kind, eta=eta.copy(), y=y.copy())
    for k, v in kw.items():
        g[k] = None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), eta.shape).copy()
    return g


def _cross(etas, ys):
    e, y = np.meshgrid(np.asarray(etas, dtype=np.float64), np.asarray(ys, dtype=np.float64), indexing="ij")
    return e.ravel(), y.ravel()


def _off_for(eta, rng):
    """Offsets with fl(eta - off) + off == eta exactly: multiples of 2^-10 of about half of eta's size."""
    off = np.round(eta * rng.uniform(0.25, 0.75, eta.shape) * 1024.0) / 1024.0
    x = eta - off
    return np.where(x + off == eta, off, 0.0)


def _split(family, link, name, eta, y, theta=None, edge=False, **kw):
    """The rows split by the gate into a fast and a reference group; reference rows whose operation order is not
    finite in w, w z or the deviance form a "nonfinite" group of their own."""
    eta, y = np.broadcast_arrays(np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64))
    full = {k: (None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64), eta.shape)) for k, v in kw.items()}
    if theta is not None:
        full["theta"] = np.broadcast_to(np.asarray(theta, dtype=np.float64), eta.shape)
    f = fast_row(family, link, eta, y, has_m=full.get("m") is not None, theta=theta)
    fin = np.all(np.isfinite(ref_order(family, link, eta, y, **{k: full.get(k) for k in ("m", "off", "pw", "theta")})), axis=0)
    out = []
    pre = "edge-" if edge else ""
    for mask, kind, label in ((f, pre + "fast", "fast"), (~f & fin, pre + "ref", "ref"), (~f & ~fin, "nonfinite", "nonfinite")):
        if mask.any():
            out.append(_grp(f"{name}/{label}", kind, eta[mask], y[mask], **{k: (None if v is None else v[mask]) for k, v in full.items()}))
    return out


N1, N8 = np.nextafter(8.0, 0.0), np.nextafter(8.0, np.inf)


def eta_mu_is_one():
    """The first eta at which the reference order's mu = 1 / (1 + exp(-eta)) is 1 (1 + e rounds to 1: e <= 2^-53,
    eta = 53 ln 2 = 36.7368...), moved up by 1e-9 relative -- millions of ulps of e -- so that a device exp an ulp
    off numpy's leaves the row on the same side."""
    eta = 53.0 * np.log(2.0)
    while 1.0 + np.exp(-eta) != 1.0:
        eta = np.nextafter(eta, np.inf)
    return eta * (1.0 + 1e-9)


def logit_grid():
    rng = np.random.default_rng(81)
    G = []
    eta = rng.uniform(-8.0, 8.0, 96)
    y = np.where(rng.uniform(size=96) < 0.5, 0.0, 1.0)
    y[::7] = rng.uniform(0.0, 1.0, y[::7].shape)
    G += _split("binomial", "logit", "dense", eta, y)
    G += _split("binomial", "logit", "dense+off+pw", eta[:48], y[:48], off=_off_for(eta[:48], rng), pw=rng.uniform(0.5, 2.0, 48))
    eta = np.concatenate([rng.uniform(8.0, 30.0, 40), -rng.uniform(8.0, 30.0, 40)])
    G += _split("binomial", "logit", "dense", eta, (rng.uniform(size=80) < 0.5).astype(np.float64))
    # the edge list
    mags = [N1, 8.0, N8, 0.0, 1e-17, 5e-324, 7.5]
    e, yy = _cross([s * a for a in mags for s in (1.0, -1.0)], [0.0, 1.0, 0.5, 0.125])
    G += _split("binomial", "logit", "gate", e, yy, edge=True)
    e, yy = _cross([N1, -N1, 8.0, -8.0, 0.0, 7.5, -7.5], [np.nextafter(1.0, 2.0), -0.25, 1.5])
    G += _split("binomial", "logit", "y-outside", e, yy, edge=True)
    # mu == 1 from eta_mu_is_one() on gives 1 / 0 in g'; exp(-eta) overflows below about -709.8
    e, yy = _cross([30.0, -30.0, 36.0, -36.0, eta_mu_is_one(), 40.0, -40.0, -700.0, -745.0, -746.0], [0.0, 1.0])
    G += _split("binomial", "logit", "far", e, yy, edge=True)
    e, yy = _cross([N1, -N1, 8.0, -8.0, 0.0, 7.5, -20.0], [0.0, 1.0])
    for pwv in (0.0, 0.5, 1e-300, 1e300):
        G += _split("binomial", "logit", f"pw={pwv:g}", e, yy, edge=True, pw=pwv)
    G += _split("binomial", "logit", "off", e, yy, edge=True, off=_off_for(e, rng) + 0.25 * (e == 0.0))
    for mv in (1.0, 7.0):
        e, yy = _cross([N1, -N1, 8.0, 0.0, 2.5, -7.5, 20.0, -20.0], [0.0, 1.0, mv, np.floor(0.5 * mv)])
        G += _split("binomial", "logit", f"m={mv:g}", e, yy, edge=True, m=mv)
    return G


def poisson_grid():
    rng = np.random.default_rng(82)
    G = []
    eta = rng.uniform(-3.0, 6.0, 96)
    y = rng.poisson(np.exp(eta)).astype(np.float64)
    G += _split("poisson", "log", "dense-counts", eta, y)
    y2 = np.exp(eta[:48]) * rng.uniform(0.5, 1.5, 48)
    G += _split("poisson", "log", "dense-real+off+pw", eta[:48], y2, off=_off_for(eta[:48], rng), pw=rng.uniform(0.5, 2.0, 48))
    eta = np.concatenate([rng.uniform(700.0, 708.0, 24), -rng.uniform(700.0, 708.0, 24)])
    G += _split("poisson", "log", "dense", eta, np.where(eta > 0, np.exp(np.minimum(eta, 705.0)) * 0.5, 0.0))
    n7 = np.nextafter(700.0, 0.0)
    ys = [0.0, 1.0, 255.0, 256.0, 255.5, 1e6, 2.2250738585072014e-308, 1e-310, 5e-324, 1e299, 1e300, 1e301]
    e, yy = _cross([n7, -n7, 700.0, -700.0, 708.0, -708.0, 0.0], ys)
    G += _split("poisson", "log", "gate", e, yy, edge=True)
    e, yy = _cross([0.0, 2.5, n7, -700.0], [0.0, 3.0, 255.0, 2.5])
    for pwv in (0.0, 0.5, 1e-300):
        G += _split("poisson", "log", f"pw={pwv:g}", e, yy, edge=True, pw=pwv)
    G += _split("poisson", "log", "overflow", [710.0, 710.0], [0.0, 1.0], edge=True)   # mu = exp(eta) = inf
    return G


def gamma_grid(link):
    rng = np.random.default_rng(83 if link == "inverse" else 84)
    G = []
    lo, hi = 1e-150, 1e150
    nb = lambda v, up: np.nextafter(v, np.inf if up else 0.0)
    yedges = [nb(lo, 0), lo, nb(lo, 1), nb(hi, 0), hi, nb(hi, 1), 0.0]
    if link == "inverse":
        eta = np.exp(rng.uniform(-3.0, 3.0, 96))
        y = rng.gamma(2.0, 0.5 / eta)
        G += _split("gamma", link, "dense", eta, y)
        G += _split("gamma", link, "dense+off+pw", eta[:48], y[:48], off=_off_for(eta[:48], rng), pw=rng.uniform(0.5, 2.0, 48))
        big = 10.0 ** rng.uniform(150.0, 152.0, 32)
        G += _split("gamma", link, "dense", eta[:32], np.where(np.arange(32) % 2 == 0, big, 1.0 / big))
        e, yy = _cross([nb(lo, 0), lo, nb(lo, 1), nb(hi, 0), hi, nb(hi, 1), 1.0, 0.0, -1.0], [1.0, 3.0])
        G += _split("gamma", link, "eta-gate", e, yy, edge=True)
        e, yy = _cross([1.0, 0.5], yedges)
        G += _split("gamma", link, "y-gate", e, yy, edge=True)
    else:
        eta = rng.uniform(-3.0, 3.0, 96)
        y = rng.gamma(2.0, 0.5 * np.exp(eta))
        G += _split("gamma", link, "dense", eta, y)
        G += _split("gamma", link, "dense+off+pw", eta[:48], y[:48], off=_off_for(eta[:48], rng), pw=rng.uniform(0.5, 2.0, 48))
        eta = np.concatenate([rng.uniform(300.0, 340.0, 16), -rng.uniform(300.0, 340.0, 16)])
        G += _split("gamma", link, "dense", eta, np.exp(eta) * rng.uniform(0.5, 1.5, 32))
        n3 = np.nextafter(300.0, 0.0)
        e, yy = _cross([n3, -n3, 300.0, -300.0, np.nextafter(300.0, 400.0), 0.0], [1.0, 1e100, 1e-100])
        G += _split("gamma", link, "eta-gate", e, yy, edge=True)
        e, yy = _cross([0.0, 1.5], yedges)
        G += _split("gamma", link, "y-gate", e, yy, edge=True)
    return G


def negbin_grid():
    rng = np.random.default_rng(85)
    G = []
    n3 = np.nextafter(300.0, 0.0)
    for theta in (1e-3, 1.0, 1e6):
        eta = rng.uniform(-3.0, 4.0, 40)
        y = rng.poisson(np.exp(eta)).astype(np.float64)
        G += _split("negbin", "log", f"dense theta={theta:g}", eta, y, theta=theta)
        eta = np.concatenate([rng.uniform(300.0, 340.0, 8), -rng.uniform(300.0, 340.0, 8)])
        G += _split("negbin", "log", f"dense theta={theta:g}", eta, np.where(eta > 0, 1e130, 0.0), theta=theta)
        e, yy = _cross([n3, -n3, 300.0, -300.0, 0.0, 2.0], [0.0, 1.0, 255.0, 256.0, 255.5, np.nextafter(1e150, 0.0), 1e150])
        G += _split("negbin", "log", f"gate theta={theta:g}", e, yy, theta=theta, edge=True)
    return G


def _valid_edges(family, link):
    """The pairs without a fast path: moderate eta plus the link's validity edge (link_row_valid)."""
    rng = np.random.default_rng(90 + len(family) * 7 + len(link))
    th = 2.5 if family == "negbin" else None
    sp = lambda name, eta, y, **kw: _split(family, link, name, eta, y, theta=th, **kw)
    if family == "binomial":
        eta = rng.uniform(-2.5, 2.5, 64) if link == "probit" else rng.uniform(-3.0, 1.5, 64)
        G = sp("dense", eta, (rng.uniform(size=64) < 0.5).astype(np.float64))
        G += sp("dense m=7", eta[:24], np.floor(rng.uniform(0, 8, 24)), m=7.0)
        G += sp("edge", [0.0, -0.0, 1e-17, -4.0, 2.0 if link == "cloglog" else 4.0], [1.0, 0.0, 1.0, 0.0, 1.0], edge=True)
        return G
    if link == "log":
        eta, edges = rng.uniform(-2.0, 3.0, 64), [0.0, 709.0, 710.0]
    elif link == "identity" and family == "gaussian":
        eta, edges = rng.uniform(-5.0, 5.0, 64), [0.0, -0.0, 1e150]
    elif link == "inverse" and family == "gaussian":
        eta, edges = rng.uniform(0.25, 4.0, 64) * np.where(rng.uniform(size=64) < 0.5, -1.0, 1.0), [1e-3, -1e-3, 0.0]
    else:   # mu > 0 (sqrt: eta > 0) is the validity edge
        eta, edges = rng.uniform(0.25, 4.0, 64), [1e-3, 1.0, 0.0, -1.0]
    mu = {"identity": eta, "log": np.exp(eta), "inverse": 1.0 / eta, "sqrt": eta * eta}[link]
    if family == "gaussian":
        y = mu + rng.normal(0.0, 1.0, 64)
    elif family in ("poisson", "negbin"):
        y = rng.poisson(mu).astype(np.float64)
    else:
        y = rng.gamma(2.0, 0.5 * mu)
    G = sp("dense", eta, y)
    G += sp("dense+off+pw", eta[:32], y[:32], off=_off_for(eta[:32], rng), pw=rng.uniform(0.5, 2.0, 32))
    G += sp("validity", edges, np.ones(len(edges)), edge=True)
    return G


def grid(family, link):
    if (family, link) == ("binomial", "logit"):
        return logit_grid()
    if (family, link) == ("poisson", "log"):
        return poisson_grid()
    if family == "gamma" and link in ("inverse", "log"):
        return gamma_grid(link)
    if (family, link) == ("negbin", "log"):
        return negbin_grid()
    return _valid_edges(family, link)


def group_args(g):
    return dict(m=g.get("m"), off=g.get("off"), pw=g.get("pw"), theta=g.get("theta"))


# ---- single rows out of a pass: the design of tests/test_gpu_rowmath.py ----
def design(g, idx, p):
    """Rows idx of group g as a pass's data: X[i, 0] = x_i = eta_i - off_i, X[i, 1 + i] = 1, beta = e_0, so that
    eta_i = fl(x_i + off_i), gram[1 + i, 1 + i] = w_i, xtwz[1 + i] = w_i z_i and gram[0, 1 + i] = w_i x_i are
    exact copies (every other product is a true zero)."""
    idx = np.asarray(idx)
    n = len(idx)
    assert 1 <= n <= p - 1
    off = None if g.get("off") is None else g["off"][idx]
    x = g["eta"][idx] - (0.0 if off is None else off)
    assert np.array_equal(x + (0.0 if off is None else off), g["eta"][idx]), "eta is not fl(x + off)"
    X = np.zeros((n, p), order="F")
    X[:, 0] = x
    X[np.arange(n), 1 + np.arange(n)] = 1.0
    beta = np.zeros(p)
    beta[0] = 1.0
    pick = lambda k: None if g.get(k) is None else g[k][idx]
    return X, g["y"][idx], pick("m"), off, pick("pw"), beta


ORACLE_PAIRS = (("binomial", "logit"), ("binomial", "probit"), ("binomial", "cloglog"), ("gaussian", "identity"),
                ("poisson", "log"), ("gamma", "inverse"))   # the pairs the C oracle knows


def oracle_rows(family, link, g):
    """(w, wz, dev) per row of group g in the oracle's operation order: pyoracle.shard_partials on one-row designs
    for the pairs the C oracle knows, ref_order (the same order in numpy) for the others."""
    if (family, link) not in ORACLE_PAIRS:
        return ref_order(family, link, g["eta"], g["y"], **group_args(g))
    import pyoracle
    n = len(g["eta"])
    out = np.empty((3, n))
    for i in range(n):
        X, y, m, off, pw, beta = design(g, [i], 2)
        r = pyoracle.shard_partials(X, y, family, link, 0, beta, m=m, offset=off, prior=pw)
        out[:, i] = r[2], r[4], r[5]   # gram[1, 1], xtwz[1], scalars[S_DEV]
    return out[0], out[1], out[2]


def oracle_stats_rows(family, link, g):
    """dict slot -> per-row values of a STATS_PAIRS group in the oracle's operation order (pearsonCalc, llBinomial and
    the R families' log-likelihood ingredients): dev, pearson, ll, aux0, aux1, sumw."""
    import pyoracle
    n = len(g["eta"])
    out = np.empty((6, n))
    for i in range(n):
        X, y, m, off, pw, beta = design(g, [i], 2)
        r = pyoracle.shard_partials(X, y, family, link, 0, beta, m=m, offset=off, prior=pw)
        out[:, i] = r[5], r[6], r[7], r[9], r[10], r[12]   # scalars[S_DEV, S_PEARSON, S_LL, S_AUX0, S_AUX1, S_SUMW]
    return dict(zip(("dev", "pearson", "ll", "aux0", "aux1", "sumw"), out))


# ---- the final statistics of a fit that stops at its start (driver.cpp glm_drive, tol >= 1): Pearson and loglik ----
def gamma_loglik64(dev, sw, logy, aux0, aux1):
    """driver.cpp family_loglik for the gamma family, in fp64 (dev: with the family factor 2)."""
    import math
    with np.errstate(all="ignore"):
        disp = np.float64(dev) / np.float64(sw)
        a = np.float64(1.0) / disp
        if not (np.isfinite(a) and a > 0):
            return float("nan")
        return float((a - 1.0) * logy - aux0 / disp - (math.lgamma(a) + a * np.log(disp)) * sw - a * aux1)


def gamma_loglik_exact(ex, idx, pw):
    """(value, scale) of the gamma log-likelihood over rows idx from the exact slot sums, in long double:
    F = (a - 1) Ly - a A0 - (lgamma(a) - a log a) sw - a A1, a = sw / dev.  The scale is the first-order propagation
    of the five sums' own scales through F plus the magnitudes of F's four terms:
    |dF/da| a (S_dev / dev + 1) + |a - 1| S_Ly + a S_A0 + a S_A1 + sum |terms|,
    dF/da = Ly - A0 - (psi(a) - log a - 1) sw - A1.  None where dev = 0 (a single row with y = mu)."""
    import mpmath
    dev, s_dev = 2 * ex["dev"][0][idx].sum(), 2 * ex["dev"][1][idx].sum()
    if not dev > 0:
        return None
    sw = ld(pw).sum()
    Ly, A0, A1 = (ex[k][0][idx].sum() for k in ("logy", "aux0", "logmu"))
    sLy, sA0, sA1 = (ex[k][1][idx].sum() for k in ("logy", "aux0", "logmu"))
    a = sw / dev
    with mpmath.workdps(30):
        am = to_mpf(a)
        lga, psi = from_mpf(mpmath.loggamma(am)), from_mpf(mpmath.digamma(am))
    terms = [(a - 1) * Ly, -a * A0, -(lga - a * np.log(a)) * sw, -a * A1]
    dFda = Ly - A0 - (psi - np.log(a) - 1) * sw - A1
    scale = np.abs(dFda) * a * (s_dev / dev + 1) + np.abs(a - 1) * sLy + a * sA0 + a * sA1 + sum(np.abs(t) for t in terms)
    return sum(terms), scale


# The bar of the gamma log-likelihood in those units: the largest bar of an input sum -- the deviance over 8 rows,
# 6 + 7 = 13 (the others: log / quotient 2, a product 1, 7 for the sum: 10) -- plus the host formula's own steps:
# lgamma held to 4 ulp (8), the log (2), seven products and sums (7): 30.
GAMMA_LOGLIK_BAR = 30.0
# The floors of the final statistics' reference rows (stats_row_ref): Pearson pw (r r) / V as the fast form's bar;
# the Poisson log-likelihood pw (y log(mu) - mu - lgamma(y + 1)): exp 2 reaching mu and, through the log's argument,
# |y| (2 + 2), the log 2, lgamma held to 4 ulp (8), four products and sums (4): 18.
POISSON_LL_FLOOR = 18.0


# ---- assertion A: the bars of the fast paths, in eps units (2^-53 S_q) ----
# First-order propagation of the primitives' stated errors through the forms rowmath.hpp documents.  One correctly
# rounded operation is 1 unit of its result; a primitive good to k ulp is 2k units (an ulp is at most 2^-52
# relative): exp_small 4, log_pos 4, rcp_pos 2, libm 2.  Bars take exp at 4 (exp_small) for every kernel.  Errors
# of shared operands are added without using their correlation.  "R(a)" below: units relative to |a|.
#
# logit (e = exp(-eta), u = 1 + e, t = rcp(u), v = e t t):
#   e 4;  u: 4 e/u + 1 <= 5;  t: 5 + 2 = 7;  v: 4 + 7 + 7 + 2 = 20
#   w = pw v: 21
#   w z = pw (v (eta - off) + (y - t)):  R(v (eta-off)) 20 + 1 + 1 = 22;  y - t: 7 |t| + 1 |y - t| <= 8 (|y| + |mu|);
#         the sum 1, pw 1:  <= 22 |V (eta-off)| + 8 (|y| + |mu|) + 2 S <= 24 S
#   dev = pw (L + (1 - y) eta), L = fma(e - (u - 1), t, log_pos(u)):  log_pos 4 |log u|; u's rounding is corrected
#         to first order; e's error 4 e reaches L as 4 e / (1 + e) <= 4 L; the fma 1:  R(L) 9;  (1 - y) eta: 2;
#         the sum 1, pw 1:  <= 9 |L| + 2 |(1-y) eta| + 2 S <= 11 S
#   pearson = pw (r r) rcp(v), r = y - t: r 8 (|y| + |mu|), squared 16 + 1; rcp(v) 20 + 2; two products 2:  41
#   ll = pw (-L [- eta]):  9 |L| + 1 (|L| + |eta|) + 1 S <= 11 S
# poisson / log (mu = exp(eta)):
#   w = pw mu: 4 + 1 = 5
#   w z = pw (mu (eta - off) + (y - mu)):  R(mu (eta-off)) 4 + 1 + 1 = 6;  y - mu: 4 |mu| + 1 |y - mu| <= 5 (|y| + |mu|);
#         the sum 1, pw 1:  <= 8 S
#   dev = pw (D0 - (y - mu)), D0 = y (log_pos(y) - eta) or ylogy[y] - y eta (the table: libm log 2, the product 1):
#         either way <= 4 (|y log y| + |y eta|) + 2 |D0|;  y - mu 5 (|y| + |mu|);  the difference 1, pw 1:
#         <= 7 S + 4 C,  C = |y log y| + |y eta|  -- the row's bar is 7 + 4 C / S (log y - eta cancels where y is near
#         mu: conditioning of the form, a function of the inputs alone; the grids keep it below 64)
# gamma / inverse (mu = rcp(eta), ye = y eta, L = log_pos(ye)):
#   mu 2;  mu^2 5;  w = pw mu^2: 6
#   w z = pw (mu^2 (eta - off) - (y - mu)):  5 + 1 + 1 = 7;  y - mu: 2 |mu| + 1 |y - mu| <= 3 (|y| + |mu|);  2:  <= 9 S
#   dev = pw (-(L - (ye - 1))):  ye 1;  L: 4 |L| + 1 (absolute: d log = d ye / ye);  ye - 1: 1 |ye| + 1 |ye - 1|
#         <= 2 (|ye| + 1);  the difference 1, pw 1:  4 |L| + 2 |ye| + 3 + 2 S <= 6 S
# gamma / log (r = exp(-eta), yr = y r):
#   w = pw: exact (1 for the long double reference's own rounding of pw mu^2 / mu^2)
#   w z = pw ((eta - off) + (yr - 1)):  eta - off 1;  yr 5;  yr - 1: 5 |yr| + 1 |yr - 1| <= 6 (|yr| + 1);  2:  <= 8 S
#   dev = pw (-(log_pos(yr) - (yr - 1))):  4 |L| + 5 (absolute) + 6 (|yr| + 1) + 2 S <= 11 S + 2 S = 13 S
# negbin / log (mu = exp(eta), r = rcp(mu + theta), t = theta r, wt = mu t, yt = y + theta):
#   mu 4;  mu + theta 5;  r 7;  t 8;  wt 4 + 8 + 1 = 13;  w = pw wt: 14
#   w z = pw (wt (eta - off) + (y - mu) t):  13 + 1 + 1 = 15;  (y - mu) t: (5 + 8 + 1) t (|y| + |mu|);  2:  <= 17 S
#   dev = pw (D0 - yt log_pos(yt r)):  D0 as Poisson's, 4 C + 2 |D0|;  yt 1;  yt r: 1 + 7 + 1 = 9;  the log: 4 |Lg| + 9
#         (absolute);  T2 = yt Lg: 6 |T2| + 9 yt;  the difference 1, pw 1:  <= 6 |T2| + 9 yt + 2 |D0| + 4 C + 2 S
#         <= 11 S + 4 C  -- the row's bar is 11 + 4 C / S
A_BARS = {
    ("binomial", "logit"): dict(w=21.0, wz=24.0, dev=11.0, pearson=41.0, ll=11.0),
    ("poisson", "log"): dict(w=5.0, wz=8.0, dev=7.0),
    ("gamma", "inverse"): dict(w=6.0, wz=9.0, dev=6.0),
    ("gamma", "log"): dict(w=1.0, wz=8.0, dev=13.0),
    ("negbin", "log"): dict(w=14.0, wz=17.0, dev=11.0),
}
# Assertion B's floor where a pair has no fast path: the largest A bar of the quantity (no reference-order row
# chains more roundings than the longest fast form) -- and, for the gaussian family, whose reference rows are short
# (V = 1), their own count with mu and g' from at most one libm call or division each:
#   mu 2;  g' 3;  g'^2 7;  V g'^2 7;  1 / (.) 8;  w = pw (.) 9  (identity: w = pw exactly, 1 for the reference's own rounding)
#   z = (eta + (y - mu) g') - off: y - mu 2 + 1, times g' 3 + 1: 7, two sums 2;  w z: 9 + 9 + 1 = 19  (identity: 4)
#   dev = pw (e e), e = y - mu: 2 (2 + 1) + 1 + 1 = 8  (identity: 4)
B_FLOOR = {q: max(b[q] for b in A_BARS.values() if q in b) for q in ("w", "wz", "dev", "pearson", "ll")}
GAUSSIAN_FLOOR = {"identity": dict(w=1.0, wz=4.0, dev=4.0), "log": dict(w=9.0, wz=19.0, dev=8.0),
                  "inverse": dict(w=9.0, wz=19.0, dev=8.0)}
MAX_BAR = 64.0


def row_bars(family, link, g, q, fast=True):
    """The A bar of quantity q for every row of group g: the constant of A_BARS -- B_FLOOR for a pair without a
    fast path -- plus, on fast rows, 4 C / S for the count families' deviance."""
    n = len(g["eta"])
    if family == "gaussian":
        return np.full(n, GAUSSIAN_FLOOR[link][q])
    if (family, link) not in A_BARS:
        return np.full(n, B_FLOOR[q])
    bar = np.full(n, A_BARS[(family, link)][q])
    if fast and q == "dev" and family in ("poisson", "negbin"):
        y, eta = ld(g["y"]), ld(g["eta"])
        s = exact(family, link, g["eta"], g["y"], **group_args(g))["dev"][1]
        pw = ld(np.ones(n) if g.get("pw") is None else g["pw"])
        with np.errstate(all="ignore"):
            c = pw * (np.where(y > 0, np.abs(y * np.log(y)), 0) + np.abs(y * eta))
            bar = bar + np.where(c > 0, 4.0 * (c / s), 0.0).astype(np.float64)
    return bar
