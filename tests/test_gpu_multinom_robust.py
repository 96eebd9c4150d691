"""The block Gram kernel (blockgram.hip) and sglm_vcov_multinom_robust against
tests/multinom_robust_reference.py; the bar is 1e-9 on scaled_err / nrel, every check prints its MARGIN.
n = 1 cannot reach the kernels through the public interface -- the evaluation before them refuses a model whose
classes do not all have positive weight -- so that case of the sweep asserts the refusal."""
import numpy as np
import pytest

import multinom_reference as M
import multinom_robust_reference as RR
from conftest import nrel
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, Multinom, _lib as L
from sparkglm_amd.frame import Frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        e.set_multinom_route("block")  # the kernel at every p <= 64, whatever the measured rule would route
        yield e


def check(label, e, c, K, type="HC0", cov=False):
    """H and the meat (cov: V too) at 0.8 B_true against the reference; the signs and the exact symmetry."""
    B = 0.8 * c["B"]
    ref = RR.robust(c["X"], c["y"], B, c["pw"], type)
    e.set_data(c["X"], c["y"], prior=c["pw"])
    H = e.multinom_pass(B, K)["H"]
    V, meat = e.vcov_multinom_robust(K, B, type)
    errs = dict(H=scaled_err(H, ref["H"]), meat=scaled_err(meat, ref["meat"]))
    if cov:
        errs["V"] = scaled_err(V, ref["cov"])
    print(f"\nMARGIN {label}: {1e-9 / max(max(errs.values()), 1e-300):.3g} (" +
          ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f"; gram {e.multinom_ms()[3]:.3f} ms)")
    p = c["X"].shape[1]
    assert all(np.array_equal(A, A.T) for A in (H, meat, V))
    for j, k in ((j, k) for j in range(K - 1) for k in range(j + 1, K - 1)):
        assert np.all(np.diag(H[j * p:(j + 1) * p, k * p:(k + 1) * p]) <= 0.0)
    assert max(errs.values()) <= 1e-9, (label, errs)
    return H, meat, V


SWEEP = sorted({(1000, p, K) for p in (5, 16, 17, 33, 48, 64) for K in (3, 8)} |
               {(1000, p, K) for K in (2, 3, 4, 8, 16) for p in (17, 64)} | {(n, 33, 4) for n in (1, 63, 65, 1000)})


@pytest.mark.parametrize("n,p,K", SWEEP)
def test_block_kernel_against_the_reference(eng, n, p, K):
    c = M.make_case(n, p, K, 2)
    if n >= K:
        return check(f"block Gram {n}x{p} K={K}", eng, c, K)
    eng.set_data(c["X"], c["y"], prior=c["pw"])
    with pytest.raises(L.IllegalArgumentException, match="every class has positive total weight"):
        eng.vcov_multinom_robust(K, 0.8 * c["B"])


def test_rows_of_weight_zero_are_as_if_deleted(eng):
    """Entries 1e150 and y out of range on them: bitwise the clean case; deleted (other workgroups): to the bar."""
    c = M.make_case(449, 17, 4, 2)
    dead = c["pw"] == 0
    full = check("weight-0 rows kept", eng, c, 4)
    X, y = c["X"].copy(order="F"), np.where(dead, 99.0, c["y"])
    X[dead, 1:] = 1e150
    eng.set_data(X, y, prior=c["pw"])
    B = 0.8 * c["B"]
    dirty = (eng.multinom_pass(B, 4)["H"],) + eng.vcov_multinom_robust(4, B)[::-1]
    live = check("weight-0 rows deleted", eng, dict(c, X=np.asfortranarray(c["X"][~dead]), y=c["y"][~dead],
                                                       pw=c["pw"][~dead]), 4)
    assert all(np.array_equal(a, b) and scaled_err(w, a) <= 1e-9 for a, b, w in zip(full, dirty, live))


def test_cancellation_rows(eng):
    """pi_y within 1e-12 of 1 (eta +-36): r_y ~ 1e-16; one-hot rows, each column judged on its rows' sum |omega| |x x'|."""
    K = 4
    etas = np.array([[36.7, 0.1, -0.2], [0.2, -0.3, 36.1], [0.3, -1.2, 0.5], [-37.0, -36.5, -36.8]])
    own = [1, 3, None, 0]
    idx, n = np.tile(np.arange(4), 40), 160
    X = np.asfortranarray(np.eye(4)[idx])
    y = np.array([(i // 4) % K if own[g] is None else own[g] for i, g in enumerate(idx)], dtype=np.float64)
    pw = 1.0 + (np.arange(n) % 3).astype(np.float64)
    ref = RR.robust(X, y, etas, pw)
    eng.set_data(X, y, prior=pw)
    _, meat = eng.vcov_multinom_robust(K, etas)
    err = float(np.max(np.abs(meat - ref["meat"]) / np.where(ref["scale"] > 0, ref["scale"], np.inf)))
    print(f"\nMARGIN cancellation rows: {1e-9 / max(err, 1e-300):.3g} (least diagonal {np.min(np.diag(ref['meat'])):.1e})")
    assert np.all(meat[ref["scale"] == 0] == 0.0) and err <= 1e-9 and 0 < np.min(np.diag(ref["meat"])) < 1e-25


@pytest.mark.parametrize("n,p,K", [(3000, 64, 3), (3000, 80, 3), (6000, 256, 3)])
def test_both_routes_match_the_reference(eng, n, p, K):
    check(f"route {n}x{p} K={K}", eng, M.make_case(n, p, K, 2), K, type="HC1", cov=True)
    assert (eng.multinom_ms()[2] == 0.0) == (p <= 64)  # the block kernel | a weight kernel and a Gram pass per pair


@pytest.mark.parametrize("p", (5, 33, 64))
def test_two_calls_are_bitwise_equal(eng, p):
    c = M.make_case(20_011, p, 8, 2)
    eng.set_data(c["X"], c["y"], prior=c["pw"])
    a, b = [eng.vcov_multinom_robust(8, 0.8 * c["B"]) + (eng.multinom_pass(0.8 * c["B"], 8)["H"],) for _ in range(2)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("type", ("HC0", "HC1"))
def test_k2_is_the_binomial_sandwich(eng, type):
    c = M.make_case(4001, 33, 2, 2)
    eng.set_data(c["X"], c["y"], prior=c["pw"])
    b = 0.8 * c["B"][:, 0]
    V, meat = eng.vcov_multinom_robust(2, b, type)
    W, wmeat = eng.vcov_robust(b, "binomial", "logit", type=type, return_meat=True)
    print(f"\nMARGIN K = 2, {type}: {1e-9 / max(scaled_err(V, W), scaled_err(meat, wmeat), 1e-300):.3g}")
    assert max(scaled_err(V, W), scaled_err(meat, wmeat)) <= 1e-9


def test_group_handle_matches_the_single_handle(eng):
    c = M.make_case(4001, 33, 3, 2)
    eng.set_data(c["X"], c["y"], prior=c["pw"])
    one = eng.vcov_multinom_robust(3, 0.8 * c["B"], "HC1")
    with Engine(devices=[0, 0]) as g:
        g.set_multinom_route("block")
        g.set_data(c["X"], c["y"], prior=c["pw"])
        two = g.vcov_multinom_robust(3, 0.8 * c["B"], "HC1")
    print(f"\nMARGIN group 4001x33: {1e-9 / max(max(map(scaled_err, two, one)), 1e-300):.3g}")
    assert max(map(scaled_err, two, one)) <= 1e-9


def test_errors(eng):
    c = M.make_case(449, 17, 4, 2)
    B = 0.8 * c["B"]
    eng.set_data(c["X"], c["y"], prior=c["pw"])
    for K, b, type, msg in ((4, B, "HC2", "HC0 or SGLM_HC1"), (4, B, "HC3", "HC0 or SGLM_HC1"),
                            (1, np.zeros(17), "HC0", "n_classes <= 16"), (17, np.zeros(272), "HC0", "n_classes <= 16")):
        with pytest.raises(L.IllegalArgumentException, match=msg):
            eng.vcov_multinom_robust(K, b, type)
    for kw in (dict(offset=np.zeros(449)), dict(m=np.ones(449))):
        eng.set_data(c["X"], c["y"], prior=c["pw"], **kw)
        with pytest.raises(L.IllegalArgumentException, match="no trials m and no offset"):
            eng.vcov_multinom_robust(4, B)
    d = M.make_case(300, 129, 9, 2)
    eng.set_data(d["X"], d["y"], prior=d["pw"])
    with pytest.raises(L.IllegalArgumentException, match=r"\(n_classes - 1\) \* p <= 1024 \(got 1032\)"):
        eng.vcov_multinom_robust(9, np.zeros(1032))
    eng.set_data(c["X"], c["y"], prior=c["pw"])  # the data and a later fit are unchanged
    assert eng.fit_multinom(4).converged


def test_wrapper_round_trip(eng):
    c = M.make_case(2000, 8, 3, 2)
    names = ["(Intercept)"] + [f"x{j}" for j in range(1, 8)]
    x = Frame({nm: c["X"][:, j].copy() for j, nm in enumerate(names)})
    labels = np.array(["bird", "ant", "cat"])[c["y"].astype(int)]  # sorted: ant < bird < cat
    yc = np.array([{0: 1, 1: 0, 2: 2}[int(v)] for v in c["y"]], dtype=np.float64)
    y, w = Frame({"animal": labels}), Frame({"w": c["pw"]})
    obj = Multinom.fit(y, x, prior=w, epsilon=1e-10)  # (the wrappers' own engine: the measured rule)
    ref = RR.robust(c["X"], yc, obj.coefs.T, c["pw"], "HC1")
    t = Multinom.coeftest(obj, y, x, prior=w, type="HC1")
    se = np.sqrt(np.diag(ref["cov"]))
    assert list(t["level"]) == ["bird"] * 8 + ["cat"] * 8 and list(t["name"]) == names * 2
    assert nrel(t["se"], se) <= 1e-9 and nrel(t["estimate"], obj.coefs.reshape(-1)) == 0.0
    assert nrel(t["stat"], obj.coefs.reshape(-1) / se) <= 1e-9 and np.all((t["pvalue"] >= 0) & (t["pvalue"] <= 1))
    assert scaled_err(Multinom.vcov(obj, y, x, prior=w), RR.robust(c["X"], yc, obj.coefs.T, c["pw"])["cov"]) <= 1e-9
