"""The pass kernels' family / link arithmetic (sparkglm_amd/csrc/rowmath.hpp), row by row, against the exact
long double values of tests/rowmath_reference.py.

How a kernel shows single rows: Engine.irls_pass(e_0) on the design of rowmath_reference.design -- x_i in
column 0, a one in column 1 + i -- returns w_i, w_i z_i and w_i x_i as exact copies in the Gram and X'Wz; the
scalars are sums over the pass's rows, so the dense groups go eight rows to a pass (any summation order of n terms
loses at most n - 1 units of eps sum S_q: 7 here) and the edge lists one row to a pass.

Every error is |got - exact| / (2^-53 S_q) (rowmath_reference: "eps units").
  A  rows on a fast path: at most the bar derived beside rowmath_reference.A_BARS from the primitives' stated
     errors -- never from a measurement; a sum over n rows adds n - 1.
  B  rows on the reference operation order: in units of eps S_q kappa, at most 4 x the oracle's own error over the
     same group (device libm and fma contraction may differ from glibc by an ulp per call either way), and
     never below the quantity's A bar.
  Rows whose reference order is not finite run alone; their non-finite pattern in w and w z is the oracle's, and
  the deviance is non-finite where the oracle's is (an infinite term leaves the compensated reduction as NaN).
  w = w z = 0 exactly at pw = 0.
  The two neighbours of every gate are rows of the edge lists; the jump across each gate is printed.

Kernels: the smallest shape of each instantiation that compiles the row functions differently.

Pearson and the log-likelihood of the three pairs with statistics forms (logit, Poisson / log, gamma / inverse),
rows without m.  Narrow logit passes carry both sums in their scalars (stats_in_pass).  Everywhere else they come
from fit_glm(tol = 1, start = e_0) on the same design: glm_drive's loop `while |deltad| > tol` starts at
deltad = 1, so that fit runs the pass at e_0, no solve (no rank needed), and the final statistics -- stats_kernel on
the eta that pass stored -- at e_0.  Logit: stats_row's fast path within the gate (A), the reference order outside
(B).  Poisson and gamma: stats_row_ref on every row (B), the log-likelihood with its per-row constants -- R's
dpois in full, pw lgamma(y + 1) included, and driver.cpp's family_loglik over sum pw log y, sum pw y / mu,
sum pw log mu and the deviance.
Not covered: the narrow kernel's Poisson and gamma <STATS = true> forms (poisson_log_row<true>,
gamma_inverse_row<true>, init_stats_const's sums in S_AUX2).  They run only in the deviance-only pass a fit
predicts to be its last (engine.cpp enqueue_pass: dev_only), after at least two solves: that does need a design
of full rank and leaves eta to the solves.

Every check prints MARGIN = bar / error (>= 1 passes) per kernel, pair, path and quantity.
"""
import functools
import math
import os

import numpy as np
import pytest

import rowmath_reference as R
from sparkglm_amd import Engine
from sparkglm_amd import _lib as L

pytestmark = pytest.mark.gpu

# name -> (p, environment at engine creation, kind of sglm_pass_kernel, fused_split of pass_kernel_for)
KERNELS = {
    "narrow-p16": (16, {}, "narrow", 1),
    "narrow-p64": (64, {}, "narrow", 1),           # block pairs, the row stage on 16 of 64 lanes; the count tables
    "K1-p70": (70, {}, "fused", 1),                # libm exp
    "K1-p256": (256, {"SGLM_FUSED_SPLIT": "0"}, "fused", 0),   # exp_small
    "K1r-p150": (150, {}, "fused-split", 1),
    "K1r-p256": (256, {}, "fused-split", 1),       # the logit deviance formed after the hand-off
    "wide-p290": (290, {}, "wide", 1),
}
DENSE_ROWS = 8
ENV_KEYS = ("SGLM_FUSED_SPLIT", "SGLM_FORCE_WIDE")


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(name):
        if name not in made:
            saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
            os.environ.update(KERNELS[name][1])
            try:
                made[name] = Engine(0)
            finally:
                for k in ENV_KEYS:
                    os.environ.pop(k, None)
                    if saved[k] is not None:
                        os.environ[k] = saved[k]
        return made[name]

    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _reference(family, link):
    """Per group of the pair's grid: the exact values, the oracle's rows, the bars -- computed once, shared."""
    out = []
    stats = (family, link) in R.STATS_PAIRS
    for g in R.grid(family, link):
        a = R.group_args(g)
        fast = g["kind"] in ("fast", "edge-fast")
        d = dict(g=g, fast=fast, orc=R.oracle_rows(family, link, g), stats=False)
        if g["kind"] != "nonfinite":
            d["ex"] = R.exact(family, link, g["eta"], g["y"], **a)
            d["bars"] = {q: R.row_bars(family, link, g, q, fast=fast) for q in ("w", "wz", "dev")}
            if stats and a["m"] is None:   # (with m the binomial statistic is Binomial(m, mu / m)'s: not covered)
                d["stats"] = True
                d["orc_stats"] = R.oracle_stats_rows(family, link, g)
                if family == "binomial":
                    d["bars"].update({q: R.row_bars(family, link, g, q, fast=fast) for q in ("pearson", "ll")})
        out.append(d)
    return out


def _chunks(n, size):
    return [np.arange(a, min(a + size, n)) for a in range(0, n, size)]


def _guarded(what, fn):
    """fn(); a HIP error ends the session: nothing more is started on this device."""
    try:
        return fn()
    except L.SGLMError as err:
        pytest.exit(f"HIP error in {what}: {err}", returncode=3)


def _run_group(e, p, family, link, g, size, fit):
    """The group through the engine, `size` rows to a pass: per row w, w z, w x; per pass the index set, the
    scalars and -- with `fit` -- (pearson, loglik) of fit_glm(tol = 1, start = e_0): glm_drive's loop
    `while |deltad| > tol` starts at deltad = 1, so that fit runs the pass at e_0, no solve, and the final statistics
    (stats_kernel on the eta the pass stored) at e_0."""
    n = len(g["eta"])
    w, wz, wx = np.empty(n), np.empty(n), np.empty(n)
    sums = []
    if g.get("theta") is not None:
        e.set_theta(float(g["theta"][0]))
    for idx in _chunks(n, min(size, p - 1)):
        X, y, m, off, pw, beta = R.design(g, idx, p)
        what = f"{family}/{link} {g['name']} rows {idx.tolist()}"
        _guarded(what, lambda: e.set_data(X, y, m=m, offset=off, prior=pw))
        gram, xtwz, s = _guarded(what, lambda: e.irls_pass(beta, family=family, link=link))
        k = 1 + np.arange(len(idx))
        w[idx], wz[idx], wx[idx] = gram[k, k], xtwz[k], gram[0, k]
        st = None
        if fit:
            f = _guarded(what, lambda: e.fit_glm(family, link, tol=1.0, start=beta))
            assert f.iter == 0
            st = (f.pearson, f.loglik)
        sums.append((idx, s.copy(), st))
    return w, wz, wx, sums


def _pattern(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 3, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 0)))


def _row(g, i):
    return {k: float(g[k][i]) for k in ("eta", "y", "m", "off", "pw", "theta") if g.get(k) is not None}


class _Report:
    """The worst error / bar of every (path, quantity), the failures, the printed margins."""

    def __init__(self, label):
        self.label, self.worst, self.fail = label, {}, []

    def add(self, path, q, err, bar, where):
        err, bar = np.atleast_1d(err), np.broadcast_to(np.atleast_1d(bar), np.atleast_1d(err).shape)
        bad = ~(err <= bar)   # a NaN error fails
        with np.errstate(all="ignore"):
            ratio = np.where(err > 0, err / np.maximum(bar, 1e-300), 0.0)
        ratio = np.where(np.isnan(err), np.inf, ratio)
        i = int(np.argmax(ratio))
        cur = self.worst.get((path, q))
        if cur is None or ratio[i] > cur[0]:
            self.worst[(path, q)] = (float(ratio[i]), float(err[i]), float(bar[i]), where(i))
        emax = self.worst.setdefault(("max", path, q), [0.0])
        emax[0] = max(emax[0], float(np.nanmax(err)) if err.size else 0.0)
        for j in np.nonzero(bad)[0][:3]:
            self.fail.append(f"{self.label} {path} {q}: error {err[j]:.4g} eps units above the bar {bar[j]:.4g} at {where(int(j))}")

    def done(self):
        for key, (ratio, err, bar, at) in sorted((k, v) for k, v in self.worst.items() if k[0] != "max"):
            path, q = key
            margin = math.inf if ratio == 0 else 1.0 / ratio
            print(f"MARGIN rowmath {self.label} {path} {q}: {margin:.3g} (worst error {err:.3g} of bar {bar:.3g}, "
                  f"largest error {self.worst[('max', path, q)][0]:.3g} eps units)")
        assert not self.fail, "\n".join(self.fail[:40])


def _check_nonfinite(rep, d, w, wz, sums, at):
    """Rows alone in their passes: w and w z are NaN / +inf / -inf where the oracle's are; the deviance is
    non-finite where the oracle's is -- it is a sum, and the compensated (Neumaier) levels of the pass's
    reduction turn an infinite term into NaN (their correction forms inf - inf); the drivers ask isfinite."""
    dev = np.array([s[L.S_DEV] for _, s, _ in sums])
    for q, got, want in zip(("w", "wz", "dev"), (w, wz, dev), d["orc"]):
        if q == "dev":
            same = (_pattern(got) != 0) == (_pattern(want) != 0)
        else:
            same = _pattern(got) == _pattern(want)
        for j in np.nonzero(~same)[0][:3]:
            rep.fail.append(f"{rep.label} nonfinite {q}: got {got[j]!r}, the oracle's order gives {want[j]!r} at {at(int(j))}")
    assert np.all(np.any(_pattern([w, wz, dev]) != 0, axis=0)), (rep.label, d["g"]["name"], "a row here is finite in the kernel")


def _check_rows(rep, path, d, fast, bars, kap, w, wz, wx, at):
    """Per row: w and w z (A, or B in units of eps S_q kappa), the Gram's w x, exact zeros at pw = 0."""
    g, ex = d["g"], d["ex"]
    for k, (q, got) in enumerate((("w", w), ("wz", wz))):
        err = R.units(got, ex[q][0], ex[q][1] * kap)
        bar = bars[q]
        if not fast:   # B: 4 x the oracle's own error over the group, the A bar its floor
            orc = R.units(d["orc"][k], ex[q][0], ex[q][1] * kap)
            bar = np.maximum(bar, 4.0 * float(orc.max()))
        rep.add(path, q, err, bar, at)
    # w x: the Gram's copy of w times x, rounded once
    x = g["eta"] - (0.0 if g.get("off") is None else g["off"])
    rep.add(path, "wx", R.units(wx, R.ld(w) * R.ld(x), np.abs(R.ld(w) * R.ld(x))), 1.0, at)
    zero = np.zeros(len(w), dtype=bool) if g.get("pw") is None else g["pw"] == 0.0
    if zero.any() and not (np.all(w[zero] == 0.0) and np.all(wz[zero] == 0.0)):
        rep.fail.append(f"{rep.label} {g['name']}: w or w z is not exactly 0 at pw = 0")
    return zero


def _check_sum(rep, path, name, fast, edge, sums, got_of, exact_q, bar_q, kap, orc_q, zero, at):
    """One scalar of the passes of a group -- a sum over each pass's rows -- in units of eps sum S_q (kappa).
    A: the rows' bars weighted by their scales, plus n - 1 for the sum.  B: that as the floor of 4 x the oracle's
    own error over the group's passes.  Where the oracle's order is past fp64's range (pw = 1e300), so is the
    kernel's value."""
    errs, brs, firsts = [], [], []
    orc_worst = 0.0
    for idx, s, st in sums:
        got = got_of(s, st)
        if not fast and not np.isfinite(math.fsum(orc_q[idx])):
            if np.isfinite(got):
                rep.fail.append(f"{rep.label} {path} {name}: {got!r} where the oracle's order overflows at {at(int(idx[0]))}")
            continue
        val, sc = exact_q[0][idx].sum(), (exact_q[1][idx] * kap[idx]).sum()
        errs.append(R.units([got], R.ld([0.0]) + val, R.ld([0.0]) + sc)[0])
        if sc > 0:
            brs.append(float((bar_q[idx] * exact_q[1][idx] * kap[idx]).sum() / sc) + (len(idx) - 1))
        else:
            brs.append(float(bar_q[idx].max()))
        firsts.append(int(idx[0]))
        if not fast:
            orc_worst = max(orc_worst, R.units([math.fsum(orc_q[idx])], R.ld([0.0]) + val, R.ld([0.0]) + sc)[0])
        if zero[idx].all() and got != 0.0:
            rep.fail.append(f"{rep.label} {path}: the {name} sum of rows with pw = 0 is {got!r} at {at(int(idx[0]))}")
    if errs:
        brs = np.array(brs)
        if not fast:
            brs = np.maximum(brs, 4.0 * orc_worst)
        rep.add(path, name if edge else (name + "-sum"), np.array(errs), brs, lambda i: at(firsts[i]))


def _check_gamma_loglik(rep, path, d, edge, sums, at):
    """The gamma log-likelihood of the fit at e_0 (driver.cpp family_loglik over the final statistics' sums and the
    deviance) against the same formula over the exact sums, in the units of rowmath_reference.gamma_loglik_exact;
    the bar: GAMMA_LOGLIK_BAR, or 4 x the error of the formula over the oracle's sums where that is larger."""
    g, ex, o = d["g"], d["ex"], d["orc_stats"]
    errs, orcs, firsts = [], [], []
    for idx, s, st in sums:
        pw = np.ones(len(idx)) if g.get("pw") is None else g["pw"][idx]
        fs = lambda k: math.fsum(o[k][idx])
        with np.errstate(all="ignore"):
            want64 = R.gamma_loglik64(2.0 * fs("dev"), fs("sumw"), fs("ll"), fs("aux0"), fs("aux1"))
        exact = R.gamma_loglik_exact(ex, idx, pw) if math.fsum(pw) > 0 else None
        if exact is None or not np.isfinite(want64):
            if np.isfinite(st[1]) and not (exact is not None and np.isfinite(float(exact[0]))):
                rep.fail.append(f"{rep.label} {path} loglik: {st[1]!r} where the formula is not finite at {at(int(idx[0]))}")
            continue
        val, sc = R.ld([0.0]) + exact[0], R.ld([0.0]) + exact[1]
        errs.append(R.units([st[1]], val, sc)[0])
        orcs.append(R.units([want64], val, sc)[0])
        firsts.append(int(idx[0]))
    if errs:
        bar = max(R.GAMMA_LOGLIK_BAR, 4.0 * max(orcs))
        rep.add(path, "loglik" if edge else "loglik-sum", np.array(errs), bar, lambda i: at(firsts[i]))


def _check_group_sums(rep, path, family, link, d, fast, edge, bars, kap, sums, zero, in_pass_stats, at):
    """The deviance of every pass; Pearson and the log-likelihood where the group carries them -- from the narrow
    logit pass's own scalars (stats_in_pass), elsewhere from the fit at e_0; sum pw and S_BAD."""
    g, ex = d["g"], d["ex"]
    ones = np.ones(len(g["eta"]), dtype=R.LD)
    args = dict(rep=rep, path=path, fast=fast, edge=edge, sums=sums, zero=zero, at=at)
    _check_sum(name="dev", got_of=lambda s, st: s[L.S_DEV], exact_q=ex["dev"], bar_q=bars["dev"], kap=kap, orc_q=d["orc"][2], **args)
    if d["stats"]:
        o = d["orc_stats"]
        if family == "binomial":
            pear = (lambda s, st: s[L.S_PEARSON]) if in_pass_stats else (lambda s, st: st[0])
            ll = (lambda s, st: s[L.S_LL]) if in_pass_stats else (lambda s, st: st[1])
            _check_sum(name="pearson", got_of=pear, exact_q=ex["pearson"], bar_q=bars["pearson"], kap=kap, orc_q=o["pearson"], **args)
            _check_sum(name="ll", got_of=ll, exact_q=ex["ll"], bar_q=bars["ll"], kap=kap, orc_q=o["ll"], **args)
        else:
            # Poisson / gamma: the final statistics run the reference order on every row (stats_row_ref): B, with
            # the floors of rowmath_reference
            n = len(g["eta"])
            ref_args = dict(args, fast=False)
            _check_sum(name="pearson", got_of=lambda s, st: st[0], exact_q=ex["pearson"], bar_q=np.full(n, R.B_FLOOR["pearson"]),
                       kap=ones, orc_q=o["pearson"], **ref_args)
            if family == "poisson":
                _check_sum(name="loglik", got_of=lambda s, st: st[1], exact_q=ex["ll_full"],
                           bar_q=np.full(n, R.POISSON_LL_FLOOR), kap=ones, orc_q=o["ll"], **ref_args)
            else:
                _check_gamma_loglik(rep, path, d, edge, sums, at)
    for idx, s, _ in sums:
        pw = np.ones(len(idx)) if g.get("pw") is None else g["pw"][idx]
        tot = R.ld([math.fsum(pw)])
        rep.add(path, "sumw", R.units([s[L.S_SUMW]], tot, tot), len(idx) - 1 + 1e-9, lambda i: at(int(idx[0])))
        if in_pass_stats and d["stats"] and s[L.S_BAD] != 0.0:
            rep.fail.append(f"{rep.label} {g['name']}: S_BAD = {s[L.S_BAD]} on rows with y in [0, 2)")


def _check_pair(e, name, family, link):
    p, _, kind, split = KERNELS[name]
    rep = _Report(f"{name} {family}/{link}")
    in_pass_stats = kind == "narrow" and (family, link) == ("binomial", "logit")
    kept = {}
    for d in _reference(family, link):
        g = d["g"]
        edge = g["kind"] not in ("fast", "ref")
        fit = d["stats"] and not in_pass_stats
        w, wz, wx, sums = _run_group(e, p, family, link, g, 1 if edge else DENSE_ROWS, fit)
        at = lambda i, g=g: (g["name"], _row(g, i))
        if g["kind"] == "nonfinite":
            _check_nonfinite(rep, d, w, wz, sums, at)
            continue
        ex, bars, fast = d["ex"], d["bars"], d["fast"]
        if fast and kind == "wide" and (family, link) == ("gamma", "log"):
            # the wide row kernels run every non-canonical pair through the run-time-link rows (wide.hip
            # launch_rows_fl): gamma / log has no fast path there, its rows are reference-order rows
            fast, bars = False, {q: np.full(len(w), R.B_FLOOR[q]) for q in bars}
        path = ("fast" if fast else "ref") + ("-edge" if edge else "")
        kap = np.ones(len(w), dtype=R.LD) if fast else ex["kappa"]
        zero = _check_rows(rep, path, d, fast, bars, kap, w, wz, wx, at)
        _check_group_sums(rep, path, family, link, d, fast, edge, bars, kap, sums, zero, in_pass_stats, at)
        if edge:
            kept[g["name"]] = (g, ex, dict(w=w, wz=wz, dev=np.array([s[L.S_DEV] for _, s, _ in sums])))
        if not fast:
            _check_reference_order(rep, path, family, link, g, d["orc"], dict(w=w, wz=wz), sums, edge, at)
    _print_gate_jumps(rep.label, kept)
    st = e.stats()
    assert st["pass_kernel_kind"] == kind, (name, st["pass_kernel_kind"], st["pass_kernel_name"])
    assert L.pass_kernel_for(1, p, family, link, fused_split=split)[0] == kind
    rep.done()


def _check_reference_order(rep, path, family, link, g, orc, got, sums, edge, at):
    """C  That a row outside its gate took the reference operation order, where the order leaves a mark no libm
    difference can: (1) where the oracle's order gives an exact zero (1 / (V g'^2) with g'^2 overflowed, say), so
    does the kernel; (2) logit edge rows with (eta > 0, y = 1) or (eta < 0, y = 0), |eta| <= 36: the row's deviance
    is log(1 / mu) or log(1 / (1 - mu)) of a quotient rounded next to 1 -- that rounding, thousands of eps of the
    deviance at |eta| = 8, is the same on both sides (an ulp of exp does not survive fl(1 + e) but once in about
    2000 rows), so kernel and oracle agree to the two logs' 2 ulp (4 units of the deviance) and the two products
    by pw (1 each): 6, where the fast form's value lies thousands away."""
    for q, o in zip(("w", "wz"), orc[:2]):
        bad = (o == 0.0) & (got[q] != 0.0)
        for j in np.nonzero(bad)[0][:3]:
            rep.fail.append(f"{rep.label} {path} {q}: {got[q][j]!r} where the reference order gives an exact 0 at {at(int(j))}")
    if (family, link) != ("binomial", "logit") or not edge or g.get("m") is not None:
        return
    eta, y = g["eta"], g["y"]
    mark = (((eta > 0) & (y == 1.0)) | ((eta < 0) & (y == 0.0))) & (np.abs(eta) <= 36.0) & (orc[2] != 0.0)
    if mark.any():
        dev = np.array([s[L.S_DEV] for _, s, _ in sums])
        rep.add(path, "dev-vs-oracle", R.units(dev[mark], R.ld(orc[2][mark]), np.abs(R.ld(orc[2][mark]))), 6.0,
                lambda i: at(int(np.nonzero(mark)[0][i])))


def _print_gate_jumps(label, kept):
    """For every fast edge row whose neighbour in eta (one ulp outward, everything else equal) is a reference edge
    row: the signed errors on both sides and their difference -- the jump across the gate -- in eps units."""
    keys = ("y", "m", "off", "pw", "theta")
    fast = [(n, v) for n, v in kept.items() if n.endswith("/fast")]
    ref = [(n, v) for n, v in kept.items() if n.endswith("/ref")]
    worst = {}
    for nf, (gf, exf, gotf) in fast:
        for nr, (gr, exr, gotr) in ref:
            if nf.rsplit("/", 1)[0] != nr.rsplit("/", 1)[0]:
                continue
            for i in range(len(gf["eta"])):
                out = np.nextafter(gf["eta"][i], np.copysign(np.inf, gf["eta"][i]))
                for j in np.nonzero(gr["eta"] == out)[0]:
                    if any((gf.get(k) is None) != (gr.get(k) is None) or (gf.get(k) is not None and gf[k][i] != gr[k][j]) for k in keys):
                        continue
                    for q in ("w", "wz", "dev"):
                        a = R.signed_units([gotf[q][i]], exf[q][0][i:i + 1], exf[q][1][i:i + 1])[0]
                        b = R.signed_units([gotr[q][j]], exr[q][0][j:j + 1], exr[q][1][j:j + 1])[0]
                        if abs(b - a) >= worst.get(q, (-1.0,))[0]:
                            worst[q] = (abs(b - a), a, b, float(gf["eta"][i]), float(gf["y"][i]))
    for q, (jump, a, b, eta, y) in sorted(worst.items()):
        print(f"GATE rowmath {label} {q}: largest jump {jump:.3g} eps units (fast side {a:+.3g}, reference side {b:+.3g}) "
              f"at eta = {eta!r}, y = {y!r}")


@pytest.mark.parametrize("family,link", R.PAIRS)
@pytest.mark.parametrize("name", list(KERNELS))
def test_rows_against_long_double(engines, name, family, link):
    _check_pair(engines(name), name, family, link)


@pytest.mark.parametrize("init", ["single", "multiple"])
def test_poisson_init_table_rows_are_the_reference_rows_bitwise(engines, init):
    """The narrow p = 64 initial pass takes the unit deviance of an integer count below 256 from its LDS table,
    built with the reference's own expressions: bit for bit what K1 (p = 70: no table, pass_row_ref on every
    row) gives for the same row.  Counts beside and past the table's edge take the reference path in both."""
    mu0 = 1.7
    ys, pws, offs = [0.0, 1.0, 2.0, 7.0, 100.0, 255.0, 256.0, 2.5], [1.0, 0.5], [0.0, 0.25]
    y, pw, off = (a.ravel() for a in np.meshgrid(ys, pws, offs, indexing="ij"))
    g = dict(name="init", kind="edge-ref", eta=0.5 + off, y=y, pw=pw, off=off)
    out = {}
    for name in ("narrow-p64", "K1-p70"):
        e, p = engines(name), KERNELS[name][0]
        rows = []
        for i in range(len(y)):
            X, yy, _, oo, pp, _ = R.design(g, [i], p)
            what = f"poisson initial pass ({init}) on {name}, row {i}"
            _guarded(what, lambda: e.set_data(X, yy, offset=oo, prior=pp))
            gram, xtwz, s = _guarded(what, lambda: e.irls_pass(None, mu0=mu0, family="poisson", link="log", init=init))
            rows.append([gram[1, 1], xtwz[1], s[L.S_DEV], s[L.S_SUMW]])
        out[name] = np.array(rows)
        assert e.stats()["pass_kernel_kind"] == KERNELS[name][2]
    a, b = out["narrow-p64"], out["K1-p70"]
    assert np.all(np.isfinite(a)) and np.all(a[:, 0] > 0)
    diff = np.nonzero(np.any(a.view(np.int64) != b.view(np.int64), axis=1))[0]
    print(f"\nPoisson initial pass ({init}): {len(y)} rows, {len(diff)} differ between the table and the reference rows")
    assert len(diff) == 0, [(_row(g, int(i)), a[i].tolist(), b[i].tolist()) for i in diff[:4]]
