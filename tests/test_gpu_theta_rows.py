"""theta_terms_kernel (sparkglm_amd/csrc/theta.hip, polygamma.hpp), row by row, against the exact values of
tests/theta_reference.py (mpmath at 60 digits, pinned at 400 by tests/test_theta_reference.py).

How the kernel shows single rows: Engine.theta_terms sums over the data set's rows, so a row is a data set of
n = 1 under the identity link -- X = [[mu]], beta = [1], no offset: eta = mu exactly, the kernel's mu is the
reference's.  Every error is |got - exact| / (2^-53 S_q), S_q the operand magnitudes of the kernel's documented last
additive step (theta_reference: "eps units"); every bar is the first-order propagation of the primitives' stated
errors written out in theta_reference -- the difference functions' 6 ulp is polygamma.hpp's statement, asserted on
the host -- never a measurement.  A sum over n rows adds n - 1.

  single rows     every grid row at every theta: score, info, loglik and mom within the row's bar; sum w = pw
  groups of 8     row bars + 7, in units of sum S
  the whole grid  one data set per theta, row bars + n - 1 in units of sum pw S, and again over its rows of moderate
                  prior weight (beside pw = 1e150 no other row is visible).  This replaces the `norm` bar of
                  test_gpu_negbin.py::test_theta_terms_against_scipy, which at theta = 1e4 is twice the whole
                  score; that a zero score fails here is asserted, on the reference alone, by
                  tests/test_theta_reference.py::test_a_zero_score_would_fail_the_whole_grid_sum
  the log link    a subset through mu = exp(eta): the bar widened by |mu dq/dmu| * 2 / S_q (exp: 1 ulp)
  the gate        y = 16 takes the finite sums, 16.5, nextafter(17, 0), 17 and 18 the difference functions.  The two
                  forms no longer differ by more than their bars (they did, from theta = 1e3 up, while the second was
                  digamma_pos(theta + y) - digamma_pos(theta)), so which one a row took cannot be read off its value;
                  instead both sides of the gate meet the finite-sum side's bar, D at 17 units
  every call twice: bitwise equal

Every check prints MARGIN = bar / error (>= 1 passes) and, per theta, how many rows of either branch miss."""
import time

import numpy as np
import pytest

import theta_reference as TR
from sparkglm_amd import Engine
from sparkglm_amd import _lib as L

pytestmark = pytest.mark.gpu

OUT = ("score", "info", "ll", "mom")   # Engine.theta_terms' first four slots; the fifth is sum w
IDS = [f"theta{t:g}" for t in TR.THETAS]


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def _terms(e, x, y, pw, theta, link):
    """theta_terms of the data set (x as the one column, beta = 1), called twice: bitwise equal.  A HIP error ends
    the session: nothing more is started on this device."""
    try:
        e.set_data(np.asarray(x, dtype=np.float64).reshape(-1, 1), y, prior=pw)
        a = e.theta_terms(np.ones(1), theta, link)
        b = e.theta_terms(np.ones(1), theta, link)
    except L.SGLMError as err:
        pytest.exit(f"HIP error in theta_terms: {err}", returncode=3)
    assert np.array_equal(a, b), (theta, link, a, b)
    return a


_SINGLE = {}


def _single_rows(e, theta):
    """The grid of theta, one row to a data set: (y, mu, pw, got[n, 5], reference) -- run once, shared."""
    if theta not in _SINGLE:
        y, mu, pw = TR.grid(theta)
        t0 = time.perf_counter()
        got = np.array([_terms(e, [mu[i]], [y[i]], [pw[i]], theta, "identity") for i in range(len(y))])
        print(f"\n{len(y)} single rows at theta {theta:g}: {time.perf_counter() - t0:.2f} s")
        _SINGLE[theta] = (y, mu, pw, got, TR.exact_rows(y, mu, pw, theta))
    return _SINGLE[theta]


def _report(label, theta, y, err, bars):
    """Print the margins and the misses per branch; return the misses (rows x quantities)."""
    miss = {q: err[q] > bars[q] for q in OUT}
    anyq = np.any([miss[q] for q in OUT], axis=0)
    fs = TR.finite_sum_row(y)
    with np.errstate(divide="ignore"):
        print(f"\nMARGIN {label} theta={theta:g}: " + ", ".join(
            f"{q} {np.min(bars[q] / np.maximum(err[q], 1e-300)):.3g} (largest error {err[q].max():.3g})" for q in OUT))
    print(f"MISSES {label} theta={theta:g}: {int(anyq.sum())} of {len(y)} rows -- finite-sum rows {int((anyq & fs).sum())} of "
          f"{int(fs.sum())}, difference rows {int((anyq & ~fs).sum())} of {int((~fs).sum())}; "
          + ", ".join(f"{q} {int(miss[q].sum())}" for q in OUT))
    return [(q, float(y[i]), float(err[q][i]), float(bars[q][i])) for q in OUT for i in np.flatnonzero(miss[q])]


@pytest.mark.parametrize("theta", TR.THETAS, ids=IDS)
def test_single_rows(eng, theta):
    y, mu, pw, got, (val, sc, bars) = _single_rows(eng, theta)
    assert np.array_equal(got[:, 4], pw)
    err = {q: TR.units(got[:, k], val[q], sc[q]) for k, q in enumerate(OUT)}
    bad = _report("single rows", theta, y, err, bars)
    # a finding, not a check: the log-likelihood row's six terms cancel at a large theta, so within its bar (units of
    # the six magnitudes) the row is this far from the exact value, relative, over the rows with |row / pw| >= 1
    big = np.abs(val["ll"]) >= pw
    rel = np.abs((got[big, 2].astype(TR.LD) - val["ll"][big]) / val["ll"][big])
    print(f"LOGLIK theta={theta:g}: largest relative distance from the exact row {float(rel.max()):.1e} "
          f"(median {float(np.median(rel)):.1e}, {int(big.sum())} rows)")
    assert not bad, (theta, len(bad), bad[:12])


@pytest.mark.parametrize("theta", TR.THETAS, ids=IDS)
def test_both_sides_of_the_finite_sum_gate(eng, theta):
    """y = 16 (finite sums) and y = 16.5, nextafter(17, 0), 17, 18 (difference functions): every one within the
    bar of the finite-sum side at y = 16 -- D and T at 16 + 1 and 16 + 4 units -- and within its own."""
    y, mu, pw, got, (val, sc, bars) = _single_rows(eng, theta)
    rows = np.flatnonzero(np.isin(y, [16.0, 16.5, TR.YS[9], 17.0, 18.0]))
    assert {True, False} == set(TR.finite_sum_row(y[rows]))
    assert TR.bar_D(16.0) == 17.0 >= TR.BAR_DIFF and TR.bar_T(16.0) == 20.0 >= TR.BAR_DIFF   # the finite side's is the wider
    fs = TR.finite_sum_row(y[rows])
    for k, q in enumerate(OUT[:2]):
        err = TR.units(got[rows, k], val[q][rows], sc[q][rows])
        # the y = 16 rows' bar where D (T) is the whole scale: 17 (20) units, and the row's three of its last step
        side = 3.0 + (TR.bar_D(16.0) if q == "score" else TR.bar_T(16.0))
        print(f"\nMARGIN gate theta={theta:g} {q}: bar {side:.1f}, finite side {side / max(err[fs].max(), 1e-300):.3g}, "
              f"difference side {side / max(err[~fs].max(), 1e-300):.3g}")
        assert np.all(bars[q][rows][~fs] <= 3.0 + TR.BAR_DIFF) and np.all(err <= side), (theta, q, err)


def _sum_check(e, label, theta, y, x, pw, ref, sets, link="identity"):
    """Each index set as one data set: every quantity within max row bar + n - 1 units of sum S."""
    val, sc, bars = ref
    bad = []
    worst = dict.fromkeys(OUT, np.inf)
    for idx in sets:
        got = _terms(e, x[idx], y[idx], pw[idx], theta, link)
        for k, q in enumerate(OUT):
            bar = bars[q][idx].max() + len(idx) - 1
            err = float(TR.units(got[k], val[q][idx].sum(), sc[q][idx].sum()))
            worst[q] = min(worst[q], bar / max(err, 1e-300))
            if err > bar:
                bad.append((q, len(idx), int(idx[0]), err, bar))
        assert abs(got[4] - pw[idx].sum()) <= len(idx) * 2.0 ** -53 * pw[idx].sum()
    print(f"\nMARGIN {label} theta={theta:g}: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items())
          + f"; MISSES {len(bad)} of {len(sets) * len(OUT)}")
    return bad


@pytest.mark.parametrize("theta", TR.THETAS, ids=IDS)
def test_groups_of_eight(eng, theta):
    """The grid's rows eight to a data set, sorted by prior weight first so that a group's rows are of one size."""
    y, mu, pw = TR.grid(theta)
    ref = TR.exact_rows(y, mu, pw, theta)
    order = np.argsort(pw, kind="stable")
    sets = [order[a:a + 8] for a in range(0, len(order), 8)]
    bad = _sum_check(eng, "groups of 8", theta, y, mu, pw, ref, sets)
    assert not bad, (theta, len(bad), bad[:12])


@pytest.mark.parametrize("theta", TR.THETAS, ids=IDS)
def test_the_whole_grid_in_one_data_set(eng, theta):
    y, mu, pw = TR.grid(theta)
    ref = TR.exact_rows(y, mu, pw, theta)
    moderate = np.flatnonzero((pw > 1e-100) & (pw < 1e100))
    bad = _sum_check(eng, "whole grid", theta, y, mu, pw, ref, [np.arange(len(y)), moderate])
    assert not bad, (theta, bad)


@pytest.mark.parametrize("theta", TR.THETAS, ids=IDS)
def test_log_link_rows(eng, theta):
    """mu = exp(eta), a rounded exp: the reference takes the exact exp of the double eta, the bar the sensitivity."""
    y, eta, pw = TR.log_subset(theta)
    val, sc, bars = TR.exact_rows(y, eta, pw, theta, log_link=True)
    got = np.array([_terms(eng, [eta[i]], [y[i]], [pw[i]], theta, "log") for i in range(len(y))])
    err = {q: TR.units(got[:, k], val[q], sc[q]) for k, q in enumerate(OUT)}
    bad = _report("log link", theta, y, err, bars)
    assert not bad, (theta, len(bad), bad[:12])
