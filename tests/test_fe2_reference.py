"""tests/fe2_reference.py against itself, on the CPU: the sweeps on the level coefficients (the engine's route)
against the explicitly demeaned rows in np.longdouble, the dense lstsq route against both, the two-way
concentrated step against the dummy-variable fit, and the evidence for the default sweep tolerance.

The table this prints (pytest -s) is quoted in DESIGN.md 4, K12: at sweep_tol = 1e-12 the downdated A and the
solve's beta sit <= 1e-11 from the longdouble reference (asserted: 100 x what was measured, and 100 x below
the project's 1e-9 bar); at 1e-10 and 1e-8 the same figures are printed, and 1e-8 is too close to the bar."""
import numpy as np
import pytest

import fe2_reference as F2
import fe_reference as FR
from conftest import nrel, rel
from sandwich_reference import scaled_err

T = 128
N, P = 1300, 20


def case(pat2, pat1="sorted", n=N, p=P, fam="poisson", lnk="log", seed=3):
    ids1, G = FR.make_ids(pat1, n, T)
    ids2, H = F2.make_ids2(pat2, ids1, G)
    c = F2.make_case2(fam, lnk, n, p, ids1, G, ids2, H, seed)
    return c, ids1, G, ids2, H, dict(m=c["m"], off=c["off"], pw=c["pw"])


@pytest.mark.parametrize("pat2", F2.PATTERNS2)
def test_patterns_and_components(pat2):
    ids1, G = FR.make_ids("sorted", N, T)
    ids2, H = F2.make_ids2(pat2, ids1, G)
    comp1, comp2, low = F2.components(ids1, ids2, G, H)
    want = dict(cycle=1, random=1, two_comp=2, nested=4, giant=1, empty=1, single=1)[pat2]
    assert len(low) == want and G + H <= 40
    assert (comp2 < 0).sum() == (1 if pat2 == "empty" else 0) and (comp1 >= 0).all()
    XD, kept = F2.dummy_design2(np.zeros((N, 0)), ids1, ids2, G, H)
    assert np.linalg.matrix_rank(XD) == XD.shape[1] == G + len(kept)  # one column per component removed: full rank


@pytest.mark.parametrize("pat2", F2.PATTERNS2)
def test_sweeps_against_the_demeaned_rows(pat2):
    """The default sweep tolerance: A (scaled) and beta of the sweeps' downdate against the rows demeaned in
    np.longdouble, at 1e-12 (asserted <= 1e-11), 1e-10 and 1e-8 (printed)."""
    c, ids1, G, ids2, H, kw = case(pat2)
    beta, alpha, gamma = c["beta"] * 0.8, c["alpha"] * 0.5 + 0.1, c["gamma"] * 0.5
    w, z, _ = F2.rows2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, "poisson", "log", **kw)
    M = np.column_stack([c["X"], z])
    Rl = F2.demean_map(M, w, ids1, ids2, G, H)
    Al, bl = F2.gram_of(Rl, w, P)
    xl = np.linalg.solve(Al, bl)
    # the dense lstsq route (the GPU tests' reference) agrees with the longdouble one far below the bars
    Ad, bd = F2.gram_of(F2.demean_lstsq(M, w, ids1, ids2, G, H), w, P)
    assert scaled_err(Ad, Al) <= 1e-13 and nrel(bd, bl) <= 1e-12
    line = []
    for tol in (1e-12, 1e-10, 1e-8):
        d = F2.downdate(c["X"], z, w, ids1, ids2, G, H, tol)
        # beta norm-wise (max |error| / max |beta|): at this non-converged point some solved coefficients are
        # near 0, and no solve bounds their element-wise relative error (conftest.coef_bound scales the same way)
        ea, eb = scaled_err(d["A"], Al), nrel(np.linalg.solve(d["A"], d["b"]), xl)
        line.append(f"tol {tol:g}: sweeps {d['sweeps']}, A {ea:.1e}, beta {eb:.1e}")
        if tol == 1e-12:
            assert ea <= 1e-11 and eb <= 1e-11, (pat2, ea, eb)
            assert np.array_equal(d["A"], d["A"].T)
            if pat2 in ("nested", "single"):
                assert d["sweeps"] == 1  # every factor-2 level is alone in its component: one sweep is exact
    print(f"\nSWEEP TOL {pat2}: " + "; ".join(line))


@pytest.mark.parametrize("pat2", ("random", "two_comp", "empty"))
def test_sweep_solution_is_the_dummy_solution_up_to_the_null_space(pat2):
    c, ids1, G, ids2, H, kw = case(pat2, p=5)
    w, z, _ = F2.rows2(c["X"], c["y"], c["beta"], c["alpha"], c["gamma"], ids1, ids2, "poisson", "log", **kw)
    M = np.column_stack([c["X"], z])
    a, cc, _ = F2.sweeps(M, w, ids1, ids2, G, H)
    Y = F2.remove_shift(np.vstack([a, cc]), ids1, ids2, G, H)
    Y0 = F2.remove_shift(F2.solve_K(M, w, ids1, ids2, G, H), ids1, ids2, G, H)
    assert nrel(Y, Y0) <= 1e-10


@pytest.mark.parametrize("fam,lnk", [("poisson", "log"), ("binomial", "logit"), ("gaussian", "identity")])
def test_two_way_concentrated_irls_is_the_dummy_irls(fam, lnk):
    """The iteration of the issue in numpy (alpha, gamma updated from Y, normalised per component) reproduces the
    dummy-variable fit: trace, beta, alpha, gamma."""
    c, ids1, G, ids2, H, kw = case("two_comp", n=900, p=4, fam=fam, lnk=lnk)
    o, kept = F2.dummy_fit2(c["X"], c["y"], ids1, ids2, G, H, fam, lnk, **kw)
    b0, a0, g0 = F2.split_coefs(o.coefs, 4, G, H, ids2, kept)
    n = len(c["y"])
    mu0 = float(np.sum(c["y"])) / n
    beta, alpha, gamma, Y = None, np.zeros(G), np.zeros(H), None
    comp1, comp2, low = F2.components(ids1, ids2, G, H)
    for it in range(o.iter):
        w, z, _ = F2.rows2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, fam, lnk, mode=0 if it else 1, mu0=mu0, **kw)
        M = np.column_stack([c["X"], z])
        a, cc, _ = F2.sweeps(M, w, ids1, ids2, G, H, Y0=Y)
        Y = (a, cc)
        d = F2.downdate(c["X"], z, w, ids1, ids2, G, H)
        beta = np.linalg.solve(d["A"], d["b"])
        alpha = alpha + a[:, 4] - a[:, :4] @ beta
        gamma = gamma + cc[:, 4] - cc[:, :4] @ beta
        shift = gamma[low]
        alpha, gamma = alpha + shift[comp1], gamma - shift[comp2]
    assert rel(beta, b0) < 1e-8 and rel(alpha, a0) < 1e-7 and np.allclose(gamma, g0, rtol=1e-7, atol=1e-9)
    assert np.all(gamma[low] == 0.0)


def test_meat_by_demeaned_rows_is_the_dummy_meat():
    c, ids1, G, ids2, H, kw = case("random", p=5)
    alpha, gamma = F2.normalise(c["alpha"] - 0.03, c["gamma"] + 0.02, ids1, ids2, G, H)
    beta = c["beta"] + 0.05
    w, z, u = F2.rows2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, "poisson", "log", **kw)
    A, _ = F2.gram_of(F2.demean_lstsq(np.column_stack([c["X"], z]), w, ids1, ids2, G, H), w, 5)
    C = np.linalg.inv(A)
    V = C @ F2.meat2(c["X"], u, w, ids1, ids2, G, H) @ C
    Vd, Cd = F2.dummy_cov2(c["X"], c["y"], beta, alpha, gamma, ids1, ids2, G, H, "poisson", "log", "HC0", False, **kw)
    assert scaled_err(C, Cd) < 1e-10 and scaled_err(0.5 * (V + V.T), Vd) < 1e-10
