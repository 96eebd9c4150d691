"""The exact per-row theta terms of the negative binomial (sparkglm_amd/csrc/theta.hip), from mpmath.

TEST INFRASTRUCTURE ONLY (a helper module of tests/test_theta_reference.py and tests/test_gpu_theta_rows.py),
built like tests/rowmath_reference.py.

exact_rows(y, mu, pw, theta) gives, for a row of fp64 inputs taken as the exact binary numbers (mu may also be an
mpf: the log link's exact exp), the mathematical value of

    D      psi(theta + y) - psi(theta)
    T      psi'(theta) - psi'(theta + y)
    score  pw (D + log(theta / (mu + theta)) + (mu - y) / (mu + theta))
    info   pw (T - mu / (theta (mu + theta)) + (mu - y) / (mu + theta)^2)
    ll     pw dnbinom(y, theta, mu, log)
    mom    pw (y / mu - 1)^2

each with its scale S_q: the sum of the magnitudes of the operands of the last additive step of the form theta.hip
documents for q -- score pw (|D| + |lq| + |e|), info pw (|T| + |q / theta| + |e / (mu + theta)|), ll the six terms
of lgamma(theta + y) - lgamma(theta) - lgamma(y + 1) + theta log theta + y log mu - (theta + y) log(mu + theta),
mom pw (|y / mu| + 1)^2 (u = y / mu - 1 with its own operands, squared).  Errors are measured as in
rowmath_reference: units(got, exact, S) = |got - exact| / (2^-53 S), "eps units".

Working precision: at theta = 1e12 the score row is O(1 / theta^2) = 1e-24 beside psi values of size log theta =
28 whose difference D, of size y / theta, is what S is made of; a value good to 0.01 unit of S = 1e-12 needs
1e-2 * 1e-16 * 1e-12 / 28 = 4e-32 relative in psi, and the info row 1e-12 times less again.  DPS = 60 leaves
fifteen digits to spare (tests/test_theta_reference.py holds the module to 0.01 unit against 400 digits).  Values
are returned as long doubles (2^-64 of |value| <= S: 0.0005 unit).
"""
from __future__ import annotations

import functools

import mpmath
import numpy as np

from rowmath_reference import EPS, LD, from_mpf, units  # noqa: F401  (units, EPS: re-exported)

DPS = 60
QUANTITIES = ("score", "info", "ll", "mom")
THETA_SUM_MAX = 17   # theta.hip: integer counts below this take the finite sums


def finite_sum_row(y):
    """theta.hip's gate: whether a count takes the exact finite sums (else the polygamma differences)."""
    y = np.asarray(y, dtype=np.float64)
    return (y < THETA_SUM_MAX) & (y == np.floor(y))


def _mp(v):
    return v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))


def exact_row_mp(y, mu, pw, theta):
    """One row in mpmath at the caller's precision: dict name -> mpf, the quantities, their scales ("S_" + q), the
    operand magnitudes the bars weigh and the sensitivities to mu ("dmu_" + q: mu dq/dmu)."""
    y, mu, pw, th = _mp(y), _mp(mu), _mp(pw), _mp(theta)
    mt = mu + th
    D = mpmath.psi(0, th + y) - mpmath.psi(0, th)
    T = mpmath.psi(1, th) - mpmath.psi(1, th + y)
    q = mu / mt
    lq = mpmath.log1p(-q) if q < 0.5 else mpmath.log(th / mt)
    e = (mu - y) / mt
    lg = [mpmath.loggamma(th + y), -mpmath.loggamma(th), -mpmath.loggamma(y + 1), th * mpmath.log(th),
          (y * mpmath.log(mu) if y != 0 else mpmath.mpf(0)), -(th + y) * mpmath.log(mt)]
    u = y / mu - 1
    o = dict(D=D, T=T, lq=lq, e=e, qt=q / th, emt=e / mt, pw=pw)
    o["score"], o["S_score"] = pw * (D + lq + e), pw * (abs(D) + abs(lq) + abs(e))
    o["info"], o["S_info"] = pw * (T - q / th + e / mt), pw * (abs(T) + abs(q / th) + abs(e / mt))
    o["ll"], o["S_ll"] = pw * mpmath.fsum(lg), pw * mpmath.fsum(abs(t) for t in lg)
    o["mom"], o["S_mom"] = pw * u * u, pw * (abs(y / mu) + 1) ** 2
    o["ll_terms"] = [abs(t) for t in lg]
    # what a relative error of the rounded arguments theta + y, y + 1 (lgamma) and theta + y, mu + theta (the last
    # term: (theta + y) d log(mu + theta)) leaves in the log-likelihood row, per unit of relative error
    o["ll_args"] = abs((th + y) * mpmath.psi(0, th + y)) + abs((y + 1) * mpmath.psi(0, y + 1)) + (th + y)
    # mu dq/dmu (the log link's mu is a rounded exp): score (y - mu)/(mu + theta)^2, info 2 (y - mu)/(mu + theta)^3,
    # ll y/mu - (theta + y)/(mu + theta) = theta (y - mu)/(mu (mu + theta)), mom -2 (y/mu - 1) y/mu^2
    o["dmu_score"] = pw * abs(mu * (y - mu) / mt ** 2)
    o["dmu_info"] = pw * abs(2 * mu * (y - mu) / mt ** 3)
    o["dmu_ll"] = pw * abs(th * (y - mu) / mt)
    o["dmu_mom"] = pw * abs(2 * u * y / mu)
    return o


# ---- the bars, in eps units (2^-53 S_q): derived, never measured ----
# First-order propagation of the primitives' stated errors through the forms theta.hip documents, as
# rowmath_reference.A_BARS.  One correctly rounded operation (add, multiply, divide: 0.5 ulp) is 1 unit of its
# result; a primitive good to k ulp is 2 k units: libm log / log1p 1 ulp = 2, lgamma held to 4 ulp = 8 (as
# rowmath_reference holds it), digamma_diff_pos / trigamma_diff_pos 6 ulp = 12 (polygamma.hpp's statement, which
# tests/test_theta_reference.py asserts on the host).  Errors of shared operands are added without using their
# correlation.  mt = mu + theta: 1.  mu is exact (identity link: eta = mu).
#   D, finite sums (ky = y terms 1 / (theta + k)): theta + k 1, the division 1: 2 per term; ky - 1 additions of
#      partial sums <= D:  ky + 1   (y = 0: D = T = 0 exactly)
#   T, finite sums: r 2, r r 2 * 2 + 1 = 5, ky - 1 additions:  ky + 4
#   D, T by the difference functions: 12
#   q = mu / mt: 2.   lq = log1p(-q) (q < 0.5): the primitive 2, q's error through -q / ((1 - q) log1p(-q)) <= 2: 6;
#      lq = log(theta / mt): the quotient 2, absolute in the log, |lq| >= log 2: 2 / 0.693 = 2.9, the primitive 2: 6
#   e = (mu - y) / mt: 1 + 1 + 1 = 3
#   score row = pw ((D + lq) + e):  bar_D |D| + 6 |lq| + 3 |e|, two additions 2 S, pw 1 S
#   info row = pw ((T - q / theta) + e / mt):  q / theta 2 + 1 = 3;  e / mt 3 + 1 + 1 = 5;
#      bar_T |T| + 3 |q / theta| + 5 |e / mt| + 3 S
#   ll row = pw (((((lgamma(theta + y) - lgamma(theta)) - lgamma(y + 1)) + theta log theta) + y log mu) -
#      (theta + y) log mt):  the three lgamma 8 each, and the rounded arguments theta + y and y + 1 (1 unit relative:
#      |x psi(x)| absolute);  theta log theta 2 + 1 = 3;  y log mu 3;  (theta + y) log mt: theta + y 1, the log 2,
#      the product 1: 4, and mt's unit, absolute in the log: theta + y;  five additions 5 S, pw 1 S:
#      8 (|lg| three times) + 3 |theta log theta| + 3 |y log mu| + 4 |(theta + y) log mt| + ll_args + 6 S
#   mom row = pw (u u), u = y / mu - 1:  y / mu 1, the difference 1 |u|: err(u) <= 2 (|y / mu| + 1) = 2 U;
#      u u: 2 U * 2 U / ... <= 4 U^2, the product 1, pw 1:  6 S
DIFF_ULP = 6.0                    # polygamma.hpp: digamma_diff_pos, trigamma_diff_pos
BAR_DIFF = 2.0 * DIFF_ULP
BAR_LQ, BAR_E, BAR_QT, BAR_EMT, BAR_LGAMMA, BAR_MOM = 6.0, 3.0, 3.0, 5.0, 8.0, 6.0
EXP_UNITS = 2.0                   # the log link: mu = exp(eta) by libm's exp, 1 ulp (rowmath_reference: "libm 2")


def bar_D(y):
    y = float(y)
    if y == 0.0:
        return 0.0
    return y + 1.0 if finite_sum_row(y) else BAR_DIFF


def bar_T(y):
    y = float(y)
    if y == 0.0:
        return 0.0
    return y + 4.0 if finite_sum_row(y) else BAR_DIFF


def row_bars_mp(y, o, log_link=False):
    """dict q -> the derived bar of one row, from exact_row_mp's output o."""
    pw = o["pw"]
    t = o["ll_terms"]
    b = dict(
        score=pw * (bar_D(y) * abs(o["D"]) + BAR_LQ * abs(o["lq"]) + BAR_E * abs(o["e"])) / o["S_score"] + 3,
        info=pw * (bar_T(y) * abs(o["T"]) + BAR_QT * abs(o["qt"]) + BAR_EMT * abs(o["emt"])) / o["S_info"] + 3,
        ll=pw * (BAR_LGAMMA * (t[0] + t[1] + t[2]) + 3 * t[3] + 3 * t[4] + 4 * t[5] + o["ll_args"]) / o["S_ll"] + 6,
        mom=mpmath.mpf(BAR_MOM))
    if log_link:   # mu carries exp's error: |mu dq/dmu| * EXP_UNITS / S_q more
        for q in QUANTITIES:
            b[q] = b[q] + EXP_UNITS * o["dmu_" + q] / o["S_" + q]
    return {q: float(v) for q, v in b.items()}


@functools.lru_cache(maxsize=None)
def _row(y, mu, pw, theta, log_link):
    """One row at DPS digits, rounded: (values, scales, bars), dicts over D, T and QUANTITIES; cached, so that the
    tests share one evaluation and leave it unchanged.  With log_link, mu is eta and the row's mu is its exact exp."""
    with mpmath.workdps(DPS):
        o = exact_row_mp(y, mpmath.exp(_mp(mu)) if log_link else mu, pw, theta)
        val = {q: from_mpf(o[q]) for q in ("D", "T") + QUANTITIES}
        sc = {q: from_mpf(o["S_" + q]) for q in QUANTITIES}
        sc["D"], sc["T"] = abs(val["D"]), abs(val["T"])
        return val, sc, row_bars_mp(y, o, log_link)


def exact_rows(y, mu, pw, theta, log_link=False):
    """(values, scales, bars): dicts q -> array over the rows (long double, long double, float)."""
    y, mu, pw = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (y, mu, pw))
    rows = [_row(float(a), float(b), float(c), float(theta), bool(log_link)) for a, b, c in zip(y, mu, pw)]
    val = {q: np.array([r[0][q] for r in rows], dtype=LD) for q in ("D", "T") + QUANTITIES}
    sc = {q: np.array([r[1][q] for r in rows], dtype=LD) for q in ("D", "T") + QUANTITIES}
    bars = {q: np.array([r[2][q] for r in rows]) for q in QUANTITIES}
    return val, sc, bars


# ---- the grids ----
THETAS = (0.01, 0.7, 9.99, 10.0, 30.0, 1e3, 1e4, 1e6, 1e8, 1e12)
# (15.5 and 16: the difference functions' own switch, where theta stops being moved up -- rows of the CPU test's
# primitive grid only; the GPU grid keeps the ten values above)
YS = (0.0, 1.0, 2.0, 15.0, 16.0, 17.0, 18.0, 0.5, 16.5, float(np.nextafter(17.0, 0.0)), 40.0, 170.0, 171.0, 255.0,
      256.0, 1e5, 1e9)
MU_FACTORS = (0.1, 0.9, 1.0 - 2.0 ** -30, 1.0, 1.1, 10.0)
MU_FIXED = (1e-8, 1e8)
PWS = (1.0, 0.3, 1e150, 1e-150)
GATE_YS = (0.0, 16.0, 17.0, 16.5, 40.0)   # at mu = theta and its two neighbours (the q < 0.5 gate)


def grid(theta):
    """(y, mu, pw) of the rows run at theta: every y with mu = y * MU_FACTORS (y > 0) and MU_FIXED, the prior
    weights cycling so that consecutive rows differ, then the gate rows mu = theta, nextafter(theta, +-inf)."""
    rows = []
    for y in YS:
        for mu in [y * f for f in MU_FACTORS if y > 0] + list(MU_FIXED):
            rows.append((y, mu))
    for y in GATE_YS:
        for mu in (float(np.nextafter(theta, 0.0)), float(theta), float(np.nextafter(theta, np.inf))):
            rows.append((y, mu))
    y, mu = (np.array(c, dtype=np.float64) for c in zip(*rows))
    # 4 weights against 8 (or 2, or 3) values of mu per y: the stride 5 walks every y through every weight
    pw = np.array([PWS[(5 * i + i // 8) % 4] for i in range(len(rows))])
    return y, mu, pw


def log_subset(theta):
    """Rows of the log-link check: one per y class (zero, finite sum, the gate's two sides, fractional, large) at
    two values of eta = log mu each, rounded to doubles: (y, eta, pw)."""
    ys = np.array([0.0, 2.0, 16.0, 17.0, 16.5, 40.0, 255.0, 1e5])
    y = np.concatenate([ys, ys])
    with np.errstate(divide="ignore"):
        eta = np.concatenate([np.log(np.maximum(ys, 0.5) * 0.9), np.log(np.maximum(ys, 0.5) * 3.0)])
    pw = np.where(np.arange(len(y)) % 3 == 0, 0.3, 1.0)
    return y, eta, pw
