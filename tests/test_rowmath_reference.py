"""tests/rowmath_reference.py against mpmath, and the conditions its grids must meet (no GPU).

The long double row functions are what tests/test_gpu_rowmath.py judges the kernels by, to a few units of
2^-53 S_q; here they are held to 0.01 of such a unit -- a hundred times finer than what they judge -- against the
textbook formulas (the reference's own operation order: mu = unlink(eta), V, g', w = pw / (V g'^2),
z = eta + (y - mu) g' - off, the family's unit deviance) evaluated by mpmath at 400 digits, where the order's
cancellations (1 - mu at |eta| = 745, say) cost nothing.  (40 digits would do for |eta| <= 40.)"""
import mpmath
import numpy as np
import pytest

import rowmath_reference as R

DPS = 400
AGREE = 0.01   # eps units


def _mpf(v):
    return mpmath.mpf(float(v))


def _textbook(family, link, eta, y, m, off, pw, theta):
    """dict q -> mpf of one row, by the reference's operation order."""
    one = mpmath.mpf(1)
    xlog = lambda a, r: mpmath.mpf(0) if a == 0 else a * mpmath.log(r)
    if family == "binomial":
        if link == "logit":
            mu = m / (1 + mpmath.exp(-eta))
            g = m / (mu * (m - mu))
        elif link == "probit":
            mu = m * mpmath.ncdf(eta)
            g = 1 / (m * mpmath.npdf(eta))
        else:
            mu = m * (1 - mpmath.exp(-mpmath.exp(eta)))
            g = 1 / ((mu - m) * mpmath.log(1 - mu / m))
        v = mu * (1 - mu / m)
        my = m - y
        dev = pw * (xlog(y, max(y, one) / mu) + xlog(my, max(my, one) / (m - mu)))
    else:
        if link == "identity":
            mu, g = eta, one
        elif link == "log":
            mu = mpmath.exp(eta)
            g = 1 / mu
        elif link == "inverse":
            mu = 1 / eta
            g = -1 / (mu * mu)
        else:
            mu = eta * eta
            g = 1 / (2 * mpmath.sqrt(mu))
        if family == "gaussian":
            v, dev = one, pw * (y - mu) ** 2
        elif family == "poisson":
            v, dev = mu, pw * (xlog(y, y / mu) - (y - mu))
        elif family == "gamma":
            v, dev = mu * mu, pw * (-(mpmath.log(y / mu) - (y - mu) / mu))
        else:
            v = mu + mu * mu / theta
            dev = pw * (xlog(y, max(y, one) / mu) - (y + theta) * mpmath.log((y + theta) / (mu + theta)))
    w = pw / (v * g * g)
    out = dict(w=w, wz=w * (eta + (y - mu) * g - off), dev=dev)
    if (family, link) in R.STATS_PAIRS:
        out["pearson"] = pw * (y - mu) ** 2 / v
    if (family, link) == ("binomial", "logit"):
        out["ll"] = pw * (mpmath.log(mu / m) if int(y) == 1 else mpmath.log(1 - mu / m))
    elif (family, link) == ("poisson", "log"):
        out["ll"] = pw * (y * mpmath.log(mu) - mu)
        out["ll_full"] = out["ll"] - pw * mpmath.loggamma(y + 1)
    elif (family, link) == ("gamma", "inverse"):
        out["aux0"] = pw * (y / mu)
        out["aux1"] = pw * mpmath.log(y / mu)
        out["logy"], out["logmu"] = pw * mpmath.log(y), pw * mpmath.log(mu)
    return out


_ld_to_mpf = R.to_mpf


@pytest.mark.parametrize("family,link", R.PAIRS)
def test_long_double_rows_agree_with_mpmath(family, link):
    worst = (0.0, None)
    with mpmath.workdps(DPS):
        for g in R.grid(family, link):
            if g["kind"] == "nonfinite":
                continue
            ex = R.exact(family, link, g["eta"], g["y"], **R.group_args(g))
            for i in range(len(g["eta"])):
                a = {k: (mpmath.mpf(1) if g.get(k) is None else _mpf(g[k][i])) for k in ("m", "pw")}
                offv = mpmath.mpf(0) if g.get("off") is None else _mpf(g["off"][i])
                th = None if g.get("theta") is None else _mpf(g["theta"][i])
                tb = _textbook(family, link, _mpf(g["eta"][i]), _mpf(g["y"][i]), a["m"], offv, a["pw"], th)
                for q, t in tb.items():
                    if q == "ll" and family == "binomial" and g.get("m") is not None:
                        continue   # with m the statistic is Binomial(m, mu / m)'s: not an in-pass quantity
                    val, s = ex[q][0][i], ex[q][1][i]
                    assert np.isfinite(val) and np.isfinite(s), (g["name"], q, g["eta"][i], g["y"][i])
                    assert s >= abs(val) * (1 - 1e-15), (g["name"], q, "S_q below |q|")
                    d = abs(_ld_to_mpf(val) - t)
                    u = 0.0 if d == 0 else float(d / (mpmath.mpf(2) ** -53 * _ld_to_mpf(s)))
                    if u > worst[0]:
                        worst = (u, (g["name"], q, g["eta"][i], g["y"][i]))
    print(f"\n{family}/{link}: long double against mpmath, worst {worst[0]:.2e} eps units at {worst[1]}")
    assert worst[0] <= AGREE, worst


@pytest.mark.parametrize("family,link", R.PAIRS)
def test_grid_conditions(family, link):
    G = R.grid(family, link)
    fastable = (family, link) in R.FAST_PAIRS
    kinds = {g["kind"] for g in G}
    assert "ref" in kinds and (not fastable or {"fast", "edge-fast", "edge-ref"} <= kinds)
    for g in G:
        a = R.group_args(g)
        n = len(g["eta"])
        f = R.fast_row(family, link, g["eta"], g["y"], has_m=a["m"] is not None, theta=a["theta"])
        # every row on the side of the gate its group is meant for, compared in fp64 as the macro does
        assert np.all(f) if g["kind"] in ("fast", "edge-fast") else not np.any(f), g["name"]
        # eta is what the kernel forms from the design: fl((eta - off) + off)
        off = np.zeros(n) if a["off"] is None else a["off"]
        assert np.array_equal((g["eta"] - off) + off, g["eta"]), g["name"]
        ro = np.array(R.ref_order(family, link, g["eta"], g["y"], **a))
        if g["kind"] == "nonfinite":
            assert np.all(np.any(~np.isfinite(ro), axis=0)), g["name"]
            orc = np.array(R.oracle_rows(family, link, g))
            assert np.all(np.any(~np.isfinite(orc), axis=0)), (g["name"], "finite in the oracle")
            continue
        ex = R.exact(family, link, g["eta"], g["y"], **a)
        for q in ("w", "wz", "dev"):
            assert np.all(np.isfinite(ex[q][0])) and np.all(np.isfinite(ex[q][1])), (g["name"], q)
            bars = R.row_bars(family, link, g, q, fast=g["kind"] in ("fast", "edge-fast"))
            assert np.all(bars <= R.MAX_BAR), (g["name"], q, float(bars.max()))
        if g["kind"] in ("ref", "edge-ref"):
            assert np.all(np.isfinite(ro)), (g["name"], "the reference order is not finite here")
    assert max(R.B_FLOOR.values()) <= R.MAX_BAR


def test_gate_values_sit_on_their_sides():
    """The edge lists hold both neighbours of every gate, each in the group of its side."""
    def where(G, eta, y=None, **kw):
        for g in G:
            for i in range(len(g["eta"])):
                if g["eta"][i] == eta and (y is None or g["y"][i] == y) and all(
                        g.get(k) is not None and g[k][i] == v for k, v in kw.items()):
                    return g["kind"]
        return None

    G = R.grid("binomial", "logit")
    for s in (1.0, -1.0):
        assert where(G, s * R.N1, 1.0) == "edge-fast" and where(G, s * 8.0, 1.0) == "edge-ref"
        assert where(G, s * R.N8, 0.0) == "edge-ref" and where(G, s * 5e-324, 0.5) == "edge-fast"
    assert where(G, R.N1, np.nextafter(1.0, 2.0)) == "edge-ref" and where(G, R.N1, 1.0, m=1.0) == "edge-ref"
    assert where(G, R.eta_mu_is_one()) == "nonfinite" and where(G, 36.0) == "edge-ref" and where(G, -700.0) == "edge-ref"
    assert where(G, -745.0) == "nonfinite" and where(G, -746.0) == "nonfinite" and where(G, 40.0) == "nonfinite"
    assert 1.0 / (1.0 + np.exp(-36.0)) < 1.0 == 1.0 / (1.0 + np.exp(-R.eta_mu_is_one()))
    G = R.grid("poisson", "log")
    n7 = np.nextafter(700.0, 0.0)
    assert where(G, -n7, 255.0) == "edge-fast" and where(G, -700.0, 255.0) == "edge-ref"
    assert where(G, n7, 1e299) == "edge-fast" and where(G, 0.0, 1e300) == "edge-ref" and where(G, 0.0, 5e-324) == "edge-fast"
    assert where(G, 0.0, 255.5) == "edge-fast" and where(G, 0.0, 256.0) == "edge-fast"
    for link, lo in (("inverse", 1e-150), ("log", 1e-150)):
        G = R.grid("gamma", link)
        e0 = 1.0 if link == "inverse" else 0.0
        assert where(G, e0, np.nextafter(lo, 1.0)) == "edge-fast" and where(G, e0, lo) in ("edge-ref", "nonfinite")
        assert where(G, e0, np.nextafter(1e150, 0.0)) == "edge-fast" and where(G, e0, 1e150) in ("edge-ref", "nonfinite")
    G = R.grid("gamma", "inverse")
    assert where(G, np.nextafter(1e-150, 1.0), 1.0) == "edge-fast" and where(G, 1e-150, 1.0) in ("edge-ref", "nonfinite")
    G = R.grid("gamma", "log")
    n3 = np.nextafter(300.0, 0.0)
    assert where(G, n3, 1.0) == "edge-fast" and where(G, 300.0, 1.0) == "edge-ref" and where(G, -300.0, 1.0) == "edge-ref"
    G = R.grid("negbin", "log")
    for th in (1e-3, 1.0, 1e6):
        assert where(G, n3, 255.0, theta=th) == "edge-fast" and where(G, 300.0, 255.0, theta=th) == "edge-ref"
        assert where(G, 0.0, np.nextafter(1e150, 0.0), theta=th) == "edge-fast" and where(G, 0.0, 1e150, theta=th) == "edge-ref"


def test_ref_order_restates_the_oracle():
    """ref_order (numpy) and the C oracle run the same operation order: the same non-finite pattern on every group,
    and values within 1e-13 relative of each other (two libms) on the finite dense reference rows (probit apart:
    scipy's erfinv against the oracle's own)."""
    for family, link in R.ORACLE_PAIRS:
        for g in R.grid(family, link):
            ro = np.array(R.ref_order(family, link, g["eta"], g["y"], **R.group_args(g)))
            orc = np.array(R.oracle_rows(family, link, g))
            assert np.array_equal(np.isnan(ro), np.isnan(orc)) and np.array_equal(np.isinf(ro), np.isinf(orc)), g["name"]
            if g["kind"] == "ref" and link != "probit":   # (probit: erfinv of scipy against the oracle's own)
                fin = np.isfinite(ro) & (orc != 0)
                assert np.all(np.abs(ro - orc)[fin] <= 1e-13 * np.abs(orc)[fin]), g["name"]


def test_units_and_design():
    g = R.grid("binomial", "logit")[1]
    X, y, m, off, pw, beta = R.design(g, [0, 3, 5], 16)
    assert X.shape == (3, 16) and np.array_equal(X @ beta + off, g["eta"][[0, 3, 5]])
    assert np.array_equal(np.nonzero(X[1])[0], [0, 2]) and X[1, 2] == 1.0
    one = R.ld([1.0])
    assert R.units([1.0 + 2.0 ** -52], one, one)[0] == 2.0 and R.units([0.0], R.ld([0.0]), R.ld([0.0]))[0] == 0.0


def test_lgamma1p_is_the_poisson_constant():
    """lgamma(y + 1), the per-fit constant the initial pass sums for the Poisson log-likelihood."""
    y = np.array([0.0, 1.0, 2.0, 5.5, 255.0, 1e6])
    got = R.lgamma1p(y)
    assert got[0] == 0 and got[1] == 0
    with mpmath.workdps(40):
        for v, g in zip(y[2:], got[2:]):
            want = mpmath.loggamma(mpmath.mpf(float(v)) + 1)
            assert abs(R.to_mpf(g) - want) <= mpmath.mpf(2) ** -62 * abs(want), v


def test_gamma_loglik_of_the_exact_sums():
    """gamma_loglik_exact is driver.cpp's family_loglik formula over the exact sums (mpmath, 40 digits), its scale at
    least the magnitude of every term; gamma_loglik64 is the same formula in fp64."""
    g = R.grid("gamma", "inverse")[0]
    idx = np.arange(8)
    ex = R.exact("gamma", "inverse", g["eta"], g["y"])
    val, scale = R.gamma_loglik_exact(ex, idx, np.ones(8))
    with mpmath.workdps(40):
        eta, y = [_mpf(v) for v in g["eta"][idx]], [_mpf(v) for v in g["y"][idx]]
        dev = 2 * sum(-(mpmath.log(b * a) - (b * a - 1)) for a, b in zip(eta, y))
        a = 8 / dev
        want = ((a - 1) * sum(mpmath.log(b) for b in y) - a * sum(b * e for e, b in zip(eta, y))
                - (mpmath.loggamma(a) - a * mpmath.log(a)) * 8 - a * sum(-mpmath.log(e) for e in eta))
        assert abs(R.to_mpf(val) - want) <= mpmath.mpf(2) ** -53 * R.to_mpf(scale) * AGREE
        assert R.to_mpf(scale) >= abs(want)
    o = {k: ex[k][0][idx].astype(np.float64).sum() for k in ("dev", "logy", "aux0", "logmu")}
    assert abs(R.gamma_loglik64(2 * o["dev"], 8.0, o["logy"], o["aux0"], o["logmu"]) - float(want)) <= 1e-12 * float(scale)
