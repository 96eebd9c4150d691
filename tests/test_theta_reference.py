"""tests/theta_reference.py against mpmath at 400 digits, the conditions its grids must meet, and the stated
accuracy of csrc/polygamma.hpp's four functions, compiled for the host (no GPU).

The module's rows are what tests/test_gpu_theta_rows.py judges theta_terms_kernel by, to a few units of 2^-53 S_q;
here they are held to 0.01 of such a unit against the textbook formulas in their ungrouped form (theta.hip's
header, lines T_SCORE / T_INFO, and dnbinom through loggamma), where every cancellation the grouping avoids is
simply paid for in digits.  The primitives' ulp bounds asserted at the end are the numbers the GPU bars are derived
from (theta_reference.DIFF_ULP): statements about primitives, checked on the host, as log_pos's is."""
import functools
import itertools
import os
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

import rowmath_reference as R
import theta_reference as TR

DPS = 400
AGREE = 0.01   # eps units


@functools.lru_cache(maxsize=None)
def _special(x):
    """psi, psi' and loggamma at the double x, at DPS digits (a grid meets few distinct theta + y)."""
    with mpmath.workdps(DPS):
        return mpmath.psi(0, x), mpmath.psi(1, x), mpmath.loggamma(x)


def _textbook(y, mu, pw, th):
    """One row by the textbook formulas, ungrouped (mpf at the caller's precision; theta + y and y + 1 exactly)."""
    mt = mu + th
    (p0, p1, lg), (q0, q1, lgy), lg1 = _special(th), _special(th + y), _special(y + 1)[2]
    score = pw * (q0 - p0 + mpmath.log(th) + 1 - mpmath.log(mt) - (y + th) / mt)
    info = pw * (-q1 + p1 - 1 / th + 2 / mt - (y + th) / mt ** 2)
    ll = pw * (lgy - lg - lg1 + th * mpmath.log(th / mt) + (y * mpmath.log(mu / mt) if y != 0 else 0))
    return dict(score=score, info=info, ll=ll, mom=pw * (y - mu) ** 2 / mu ** 2)


@pytest.mark.parametrize("theta", TR.THETAS, ids=lambda t: f"theta{t:g}")
def test_rows_agree_with_the_textbook_at_400_digits(theta):
    worst = dict.fromkeys(TR.QUANTITIES, 0.0)
    cases = [(TR.grid(theta), False), (TR.log_subset(theta), True)]
    for (y, mu, pw), log_link in cases:
        val, sc, bars = TR.exact_rows(y, mu, pw, theta, log_link)
        with mpmath.workdps(DPS):
            for i in range(len(y)):
                m = mpmath.exp(mpmath.mpf(float(mu[i]))) if log_link else mpmath.mpf(float(mu[i]))
                want = _textbook(mpmath.mpf(float(y[i])), m, mpmath.mpf(float(pw[i])), mpmath.mpf(theta))
                for q in TR.QUANTITIES:
                    s = R.to_mpf(sc[q][i])
                    assert s > 0 and mpmath.isfinite(s), (q, theta, y[i], mu[i])
                    err = float(abs(R.to_mpf(val[q][i]) - want[q]) / (mpmath.ldexp(s, -53)))
                    worst[q] = max(worst[q], err)
                    assert err <= AGREE, (q, theta, y[i], mu[i], pw[i], err)
    print(f"\ntheta {theta:g}: module against 400 digits, worst " + ", ".join(f"{q} {v:.1e}" for q, v in worst.items()))


def test_the_grids_meet_their_conditions():
    for theta in TR.THETAS:
        y, mu, pw = TR.grid(theta)
        assert 100 <= len(y) <= 400
        assert np.all(mu > 0) and np.all(np.isfinite(mu)) and np.all(y >= 0)
        val, sc, bars = TR.exact_rows(y, mu, pw, theta)
        for q in ("D", "T") + TR.QUANTITIES:   # the reference alone is finite on every row
            assert np.all(np.isfinite(val[q])) and np.all(np.isfinite(sc[q])), (theta, q)
        for q in TR.QUANTITIES:
            assert np.all(np.isfinite(bars[q])) and np.all(bars[q] >= 3.0), (theta, q)
        # every y of the list, on both sides of the finite-sum gate, with every prior weight
        assert set(y) == set(TR.YS)
        fs = TR.finite_sum_row(y)
        assert {16.0} <= set(y[fs]) and {17.0, 16.5, TR.YS[9]} <= set(y[~fs]) and TR.YS[9] < 17.0
        for v in TR.YS:
            assert set(pw[y == v]) == set(TR.PWS), (theta, v)
        # the q < 0.5 gate: mu / (mu + theta) in fp64, as the kernel forms it -- both sides, and its neighbours
        qk = mu / (mu + theta)
        assert (qk < 0.5).any() and (qk >= 0.5).any()
        for m in (np.nextafter(theta, 0.0), theta, np.nextafter(theta, np.inf)):
            assert set(y[mu == m]) >= set(TR.GATE_YS)
        # (the bars of the log-likelihood stay moderate: the rounded arguments never dominate the row's scale)
        print(f"\ntheta {theta:g}: {len(y)} rows, largest bars " + ", ".join(f"{q} {bars[q].max():.1f}" for q in TR.QUANTITIES))
        assert bars["score"].max() <= 3 + max(TR.BAR_DIFF, 17.0) and bars["info"].max() <= 3 + max(TR.BAR_DIFF, 20.0)
        assert bars["ll"].max() <= 64.0 and bars["mom"].max() == TR.BAR_MOM


@pytest.mark.parametrize("theta", [1e4, 1e6])
def test_a_zero_score_would_fail_the_whole_grid_sum(theta):
    """The sum check over the whole grid (row bars + n - 1, in units of sum pw S) is not blind where the old
    `norm` bar was: the exact sum itself is larger than the bar, so a kernel that returned 0 fails it -- for the
    whole grid and for its rows of moderate prior weight."""
    y, mu, pw = TR.grid(theta)
    val, sc, bars = TR.exact_rows(y, mu, pw, theta)
    for rows in (np.ones(len(y), dtype=bool), (pw > 1e-100) & (pw < 1e100)):
        for q in ("score", "info"):
            bar = bars[q][rows].max() + rows.sum() - 1
            zero = float(np.abs(val[q][rows].sum()) / (R.LD(R.EPS) * sc[q][rows].sum()))
            print(f"\ntheta {theta:g} {q}: a zero sum is {zero:.3g} units off, the bar is {bar:.1f}")
            assert zero > 100 * bar


# ---- csrc/polygamma.hpp on the host ----
SRC = r'''
#include <cstdio>
#include "polygamma.hpp"
int main() {
  double a, b;
  while (std::scanf("%lf %lf", &a, &b) == 2)
    std::printf("%.17g %.17g %.17g %.17g\n", sglm::digamma_pos(a), sglm::trigamma_pos(a), sglm::digamma_diff_pos(a, b),
                sglm::trigamma_diff_pos(a, b));
  return 0;
}
'''
# polygamma.hpp's statements, in ulp
DIGAMMA_ULP, TRIGAMMA_ULP = 8.0, 5.0


@pytest.fixture(scope="module")
def host_polygamma(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("pg")
    (d / "pg.cpp").write_text(SRC)
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(root, "sparkglm_amd", "csrc"), str(d / "pg.cpp"), "-o",
                    str(d / "pg")], check=True)

    def run(pairs):
        text = "".join(f"{float(a)!r} {float(b)!r}\n" for a, b in pairs)
        out = subprocess.run([str(d / "pg")], input=text, check=True, capture_output=True, text=True, timeout=60).stdout
        got = np.array([[float(t) for t in ln.split()] for ln in out.split("\n") if ln.strip()])
        assert got.shape == (len(pairs), 4)
        return got
    return run


def _ulps(got, exact, floor=None):
    """|got - exact| in ulp of exact (2^-52 of its magnitude at the most), of max(|exact|, floor) with a floor."""
    den = abs(exact) if floor is None else max(abs(exact), floor)
    return float(abs(mpmath.mpf(float(got)) - exact) / mpmath.ldexp(den, -52))


def test_digamma_and_trigamma_meet_their_stated_ulp(host_polygamma):
    rng = np.random.default_rng(7)
    xs = np.concatenate([10.0 ** rng.uniform(-12, 12, 700), rng.uniform(0.0, 12.0, 500),   # dense below the switch
                         [1e-150, 1e-8, 0.01, 0.5, 1.0, 1.4616321449683622, 2.0, 5.999, 6.0, np.nextafter(10.0, 0.0),
                          10.0, 30.0, 170.01, 1e4, 1e6, 1e12]])
    xs = xs[xs > 0]
    got = host_polygamma([(x, 0.0) for x in xs])
    w = [0.0, 0.0]
    with mpmath.workdps(50):
        for x, g in zip(xs, got):
            w[0] = max(w[0], _ulps(g[0], mpmath.psi(0, mpmath.mpf(float(x))), floor=1))
            w[1] = max(w[1], _ulps(g[1], mpmath.psi(1, mpmath.mpf(float(x)))))
    print(f"\ndigamma_pos {w[0]:.2f} ulp of max(|psi|, 1) (stated {DIGAMMA_ULP:g}), trigamma_pos {w[1]:.2f} ulp "
          f"(stated {TRIGAMMA_ULP:g})")
    assert w[0] <= DIGAMMA_ULP and w[1] <= TRIGAMMA_ULP


def test_the_difference_functions_meet_their_stated_ulp(host_polygamma):
    """digamma_diff_pos / trigamma_diff_pos over the GPU grid's (theta, y), theta dense over [0.01, 1e12] and around
    the switch at 16 (where theta stops being moved up), y down to 2^-20; exact zeros at y = 0; NaN outside."""
    rng = np.random.default_rng(8)
    n16, p16 = np.nextafter(16.0, 0.0), np.nextafter(16.0, np.inf)
    ths = np.concatenate([TR.THETAS, [15.0, 15.5, n16, 16.0, p16, 16.5, 0.99, 1.0], 10.0 ** rng.uniform(-2, 12, 60),
                          rng.uniform(14.0, 18.0, 12), 16.0 - rng.uniform(0, 16, 12)])
    ys = np.concatenate([TR.YS, [2.0 ** -20, 1e-3, 0.25], 10.0 ** rng.uniform(-6, 9, 12)])
    pairs = list(itertools.product(ths, ys))
    got = host_polygamma(pairs)
    w, at = [0.0, 0.0], [None, None]
    with mpmath.workdps(50):
        for (a, b), g in zip(pairs, got):
            if b == 0.0:
                assert g[2] == 0.0 and g[3] == 0.0
                continue
            a, b = mpmath.mpf(float(a)), mpmath.mpf(float(b))
            ex = (mpmath.psi(0, a + b) - mpmath.psi(0, a), mpmath.psi(1, a) - mpmath.psi(1, a + b))
            for k in (0, 1):
                u = _ulps(g[2 + k], ex[k])
                if u > w[k]:
                    w[k], at[k] = u, (float(a), float(b))
    print(f"\ndigamma_diff_pos {w[0]:.2f} ulp at {at[0]}, trigamma_diff_pos {w[1]:.2f} ulp at {at[1]} (stated {TR.DIFF_ULP:g})")
    assert w[0] <= TR.DIFF_ULP and w[1] <= TR.DIFF_ULP
    bad = host_polygamma([(0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (2.0, -1.0), (2.0, float("inf")),
                          (2.0, float("nan")), (-1e300, 3.0)])
    assert np.all(np.isnan(bad[:, 2:]))
