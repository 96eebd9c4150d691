"""The cluster-robust covariance on the GPU (sglm_vcov_cluster: the signed-score kernel of influence.hip,
the segment-sum and combine kernels of cluster.hip, a Gram pass over the cluster sums) against
tests/cluster_reference.py, a numpy reference built by another route (QR for C, np.add.at for S, BLAS
for M).

Error metric: e = max_ij |V - V_ref|_ij / sqrt(V_ref,ii V_ref,jj)  (sandwich_reference.scaled_err).

Bars: those of tests/test_gpu_sandwich.py with k = 0
  V     e <= 2 max(1e-9, K_BOUND cond eps): the bread's bar, twice because C enters twice
  meat  e <= 1e-9

The reference's own error, measured on the CPU (tests/test_cluster_api.py asserts it at 3001 x 20):
fp64 against np.longdouble and against the rows summed in reverse order, meat <= 7.2e-15 and V <= 6.6e-15
on the logit designs 6007 x 20, 6007 x 129, 2049 x 256 for every id pattern; the meat's smallest-to-largest
diagonal ratio is >= 1e-4.  So the 1e-9 bar has > 1e5 of margin from the reference alone.

G = 1, and G = 2 at a converged beta, are not tested: the cluster sums cancel there (sum_i u_i x_i = 0
at the MLE) and the metric's denominator collapses.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import cluster_reference as CR
from conftest import K_BOUND, gram_cond, iris_design
from sandwich_reference import scaled_err
from sparkglm_amd import Engine, _lib as L, synth
from sparkglm_amd import distributed as D
from test_gpu_sandwich import family_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
T = L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0]  # the engine's tile_rows (no device)


def v_bar(cond):
    return 2.0 * max(1e-9, K_BOUND * cond * EPS)


def check(label, eng, X, y, beta, fam, lnk, cond, ids, G, types=("HC0", "HC1"), cadjusts=(True,), **kw):
    """set_clusters + vcov_cluster against the reference, for every (type, cadjust); {(type, cadjust): (V, M)}"""
    eng.set_clusters(ids, G)
    out = {}
    for t in types:
        for ca in cadjusts:
            ref = CR.cluster_cov(X, y, beta, fam, lnk, ids, G, t, ca, **kw)
            V, M = eng.vcov_cluster(beta, fam, lnk, type=t, cadjust=ca, return_meat=True)
            assert np.array_equal(V, V.T), (label, t, ca)
            e_v, e_m = scaled_err(V, ref["V"]), scaled_err(M, ref["M"])
            bar_v, bar_m = v_bar(cond), 1e-9
            print(f"\nMARGIN {label} {t} cadjust={ca}: {min(bar_v / max(e_v, 1e-300), bar_m / max(e_m, 1e-300)):.3g} "
                  f"(V: bar {bar_v:.2e} err {e_v:.2e}; meat: bar {bar_m:.2e} err {e_m:.2e}; cond {cond:.2e}, G {G})")
            assert e_v <= bar_v, (label, t, ca, e_v, bar_v)
            assert e_m <= bar_m, (label, t, ca, e_m, bar_m)
            out[(t, ca)] = (V, M)
    return out


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def logit(eng, n, p):
    X, y, _, _ = synth.generate(0, 0, n, p, 7 + p)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit", max_iter=3)
    return X, y, f.coefs, gram_cond(eng, f.coefs)


SWEEP_P = (1, 5, 16, 17, 20, 33, 64, 65, 129, 256)


@pytest.mark.parametrize("p", SWEEP_P)
def test_shape_sweep_logit(eng, p):
    """Every width of the score kernel and of the Gram pass over S, one to four 64-column slabs with and
    without idle lanes, rows that are no multiple of 32 / of the tile, runs around 16, 64 and the tile."""
    cadj = (True, False) if p in (20, 129) else (True,)
    # (p = 1: 8 p + 1 rows would hold two clusters, whose sums cancel at a converged beta)
    n_small = 8 * p + 1 if p > 1 else 16
    n_big = 2 * T + 1000 + 15 * (p % 7)
    assert n_big % T != 0  # the last tile is partial
    for n, patterns in ((n_small, ("two_level",)), (n_big, ("sorted", "shuffled"))):
        X, y, beta, cond = logit(eng, n, p)
        for pat in patterns:
            ids, G = CR.make_ids(pat, n, T)
            assert G >= 3
            check(f"sweep {n}x{p} {pat}", eng, X, y, beta, "binomial", "logit", cond, ids, G, cadjusts=cadj)


@pytest.mark.parametrize("p", (20, 129))
def test_singletons_give_the_hc0_meat(eng, p):
    n = 2 * T + 1000
    X, y, beta, cond = logit(eng, n, p)
    ids, G = CR.make_ids("singletons", n, T)
    out = check(f"singletons {n}x{p}", eng, X, y, beta, "binomial", "logit", cond, ids, G, types=("HC0",),
                cadjusts=(False,))
    V0, M0 = eng.vcov_robust(beta, "binomial", "logit", type="HC0", return_meat=True)
    V, M = out[("HC0", False)]
    assert scaled_err(M, M0) <= 1e-9
    assert scaled_err(V, V0) <= v_bar(cond)


@pytest.mark.parametrize("pat", ("interleaved", "two_level"))
def test_many_one_row_segments(eng, pat):
    n, p = 2 * T + 1000, 65
    X, y, beta, cond = logit(eng, n, p)
    ids, G = CR.make_ids(pat, n, T)
    check(f"{pat} {n}x{p}", eng, X, y, beta, "binomial", "logit", cond, ids, G)


def test_combine_levels(eng):
    """Clusters of 1, of more than 64 and of more than 64^2 segments side by side: the combine sums
    chunks of 64 segments level by level (one, two and three levels)."""
    n, p = 160_001, 5
    X, y, beta, cond = logit(eng, n, p)
    i = np.arange(n)
    ids = np.where(i % 2 == 0, 0, 1 + (i // 2) % 50)  # cluster 0: 80 001 one-row segments; the others 1600
    ids[-1] = 51  # one segment
    _, start, _ = L.cluster_plan(ids, 52)
    assert len(start) - 1 == n
    check("combine levels", eng, X, y, beta, "binomial", "logit", cond, ids, 52)
    ids, G = CR.make_ids("interleaved", n, T)  # 37 clusters of 4325 segments
    check("combine levels interleaved", eng, X, y, beta, "binomial", "logit", cond, ids, G)


@pytest.mark.parametrize("name", ["binomial/logit", "binomial/probit", "binomial/cloglog", "poisson", "gamma",
                                  "gaussian", "poisson/sqrt"])
def test_every_family_link(eng, name):
    """The pairs of the sandwich tests at 3001 x 20: binomial with trials m, poisson with offset and prior."""
    X, y, kw, fam, lnk = family_case(name)
    eng.set_data(X, y, m=kw.get("m"), offset=kw.get("off"), prior=kw.get("pw"))
    f = eng.fit_glm(fam, lnk)
    cond = gram_cond(eng, f.coefs, fam, lnk)
    ids, G = CR.make_ids("two_level", len(y), T)
    check(name, eng, X, y, f.coefs, fam, lnk, cond, ids, G, **kw)


def test_zero_prior_weights(eng):
    """A block of rows of weight 0: their ids stay in place, their u is exactly 0."""
    n = 3001
    X, y, off, prior = synth.generate(2, 0, n, 20, 6)
    prior = prior.copy()
    dead = (np.arange(n) >= 700) & (np.arange(n) < 1100)
    prior[dead] = 0.0
    eng.set_data(X, y, offset=off, prior=prior)
    f = eng.fit_glm("poisson", "log")
    cond = gram_cond(eng, f.coefs, "poisson", "log")
    ids, G = CR.make_ids("two_level", n, T)
    full = check("zero prior", eng, X, y, f.coefs, "poisson", "log", cond, ids, G, off=off, pw=prior)
    ref = CR.cluster_cov(X, y, f.coefs, "poisson", "log", ids, G, "HC0", True, off=off, pw=prior)
    assert np.all(ref["u"][dead] == 0.0)
    # without those rows (and their ids): the same sums, so the same meat and HC0 covariance
    keep = ~dead
    eng.set_data(np.asfortranarray(X[keep]), y[keep], offset=off[keep], prior=prior[keep])
    eng.set_clusters(ids[keep], G)
    V, M = eng.vcov_cluster(f.coefs, "poisson", "log", type="HC0", return_meat=True)
    assert scaled_err(M, full[("HC0", True)][1]) <= 1e-9
    assert scaled_err(V, full[("HC0", True)][0]) <= v_bar(cond)


def test_lm_on_iris_and_glm_coeftest(iris):
    from scipy import stats
    from sparkglm_amd.frame import Frame
    from sparkglm_amd.glm import GLM
    from sparkglm_amd.lm import LM
    X, y, names = iris_design(iris)
    xf, yf = Frame({n: X[:, j] for j, n in enumerate(names)}), Frame({"y": y})
    species = Frame({"Species": iris["Species"]})
    obj = LM.fit(xf, yf)
    beta = np.asarray(obj.coefs).reshape(-1)
    cond = float(np.linalg.cond(X.T @ X))
    labels, ids = np.unique(iris["Species"], return_inverse=True)
    assert len(labels) == 3
    for t, ca in (("HC1", True), ("HC0", False)):
        ref = CR.cluster_cov(X, y, beta, "gaussian", "identity", ids, 3, t, ca)
        V = LM.vcov_cluster(obj, xf, yf, species, type=t, cadjust=ca)
        err = scaled_err(V, ref["V"])
        print(f"\nMARGIN LM iris {t} cadjust={ca}: {v_bar(cond) / max(err, 1e-300):.3g}")
        assert err <= v_bar(cond) and np.array_equal(V, V.T)
    ref = CR.cluster_cov(X, y, beta, "gaussian", "identity", ids, 3, "HC1", True)
    tab = LM.coeftest(obj, xf, yf, type="HC1", cluster=species)
    se = np.sqrt(np.diag(ref["V"]))
    assert list(tab["name"]) == names and np.array_equal(tab["estimate"], beta)
    assert np.all(np.abs(tab["se"] - se) <= v_bar(cond) * se)
    assert np.array_equal(tab["stat"], beta / tab["se"])
    assert np.allclose(tab["pvalue"], 2.0 * stats.t.sf(np.abs(tab["stat"]), len(y) - 4), rtol=0, atol=1e-12)

    n, p = 3001, 5
    Xg, yg, _, _ = synth.generate(0, 0, n, p, 2)
    gn = [f"x{j}" for j in range(p)]
    xg, ygf = Frame({c: Xg[:, j] for j, c in enumerate(gn)}), Frame({"y": yg})
    firm = np.array([f"firm{(i // 5) % 101:03d}" for i in range(n)])  # string labels, factorised by the engine
    gobj = GLM.fit(ygf, xg, "binomial", "logit")
    gb = np.asarray(gobj.coefs).reshape(-1)
    _, gid = np.unique(firm, return_inverse=True)
    gref = CR.cluster_cov(Xg, yg, gb, "binomial", "logit", gid, 101, "HC1", True)
    gt = GLM.coeftest(gobj, ygf, xg, type="HC1", cluster=Frame({"firm": firm}))
    gse = np.sqrt(np.diag(gref["V"]))
    mu = 1.0 / (1.0 + np.exp(-(Xg @ gb)))
    gcond = float(np.linalg.cond(Xg.T @ ((mu * (1.0 - mu))[:, None] * Xg)))
    assert list(gt["name"]) == gn
    assert np.all(np.abs(gt["se"] - gse) <= v_bar(gcond) * gse)
    assert np.array_equal(gt["stat"], gb / gt["se"])
    assert np.allclose(gt["pvalue"], 2.0 * stats.norm.sf(np.abs(gt["stat"])), rtol=0, atol=1e-12)
    Vg = GLM.vcov_cluster(gobj, ygf, xg, Frame({"firm": firm}), type="HC0", cadjust=True)  # Stata's glm rule
    want = CR.cluster_cov(Xg, yg, gb, "binomial", "logit", gid, 101, "HC0", True)["V"]
    assert scaled_err(Vg, want) <= v_bar(gcond)


N_BIG, P_BIG = 20_001, 64


@pytest.fixture(scope="module")
def big(eng):
    X, y, _, _ = synth.generate(0, 0, N_BIG, P_BIG, 21)
    eng.set_data(X, y)
    f = eng.fit_glm("binomial", "logit")
    cond = gram_cond(eng, f.coefs)
    # interleaved: every cluster spans every shard; sorted: a cluster lives on one shard (but for the one
    # cut by the shard boundary), so each shard's S has rows that only the other shard fills
    pats = {}
    for pat in ("interleaved", "sorted"):
        ids, G = CR.make_ids(pat, N_BIG, T)
        pats[pat] = (ids, G, check(f"big {pat}", eng, X, y, f.coefs, "binomial", "logit", cond, ids, G))
    return X, y, f, cond, pats


def test_two_calls_are_bitwise_identical_and_the_shard_is_untouched(eng, big):
    X, y, f, cond, pats = big
    ids, G, one = pats["interleaved"]
    eng.set_data(X, y)
    eng.set_clusters(ids, G)
    before = eng.get_data()[:2]
    fit0 = eng.fit_glm("binomial", "logit")
    name = eng.stats()["pass_kernel_name"]
    for t in ("HC0", "HC1"):
        V, M = eng.vcov_cluster(f.coefs, "binomial", "logit", type=t, return_meat=True)
        assert np.array_equal(V, one[(t, True)][0]) and np.array_equal(M, one[(t, True)][1]), t
    assert np.array_equal(eng.vcov_cluster(f.coefs, "binomial", "logit", type="HC0"), one[("HC0", True)][0])
    assert eng.stats()["pass_kernel_name"] == name  # the fit's kernel record is the fit's
    ms = eng.cluster_ms()
    assert len(ms) == 4 and all(v > 0.0 for v in ms)
    after = eng.get_data()[:2]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(before[0], X) and np.array_equal(before[1], y)
    fit1 = eng.fit_glm("binomial", "logit")
    assert np.array_equal(fit0.coefs, fit1.coefs) and np.array_equal(fit0.stderr, fit1.stderr)
    assert fit0.deviance == fit1.deviance and fit0.iter == fit1.iter
    # the clusters outlive a fit, and clearing them is refused afterwards
    eng.set_clusters(None)
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.vcov_cluster(f.coefs, "binomial", "logit")


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
@pytest.mark.parametrize("devices", ([0, 0], [0]))
def test_group_handle_matches_the_single_handle(big, devices, pat):
    """[0, 0]: two shards summed on the host in shard order; [0]: the RCCL group all-reduce.  Call after
    call: the cross-shard sum lands in each shard's S, and must not reach the next call's sum."""
    X, y, f, cond, pats = big
    ids, G, one = pats[pat]
    with Engine(devices=devices) as g:
        assert g.cluster_ms() == (-1.0, -1.0, -1.0, -1.0)
        g.set_data(X, y)
        g.set_clusters(ids, G)
        first = {}
        for t in ("HC0", "HC1", "HC0", "HC1"):  # HC1: n is the global row count
            V, M = g.vcov_cluster(f.coefs, "binomial", "logit", type=t, return_meat=True)
            assert scaled_err(M, one[(t, True)][1]) <= 1e-9, t
            assert scaled_err(V, one[(t, True)][0]) <= v_bar(cond), t
            assert np.array_equal(V, V.T)
            if t in first:
                assert np.array_equal(V, first[t][0]) and np.array_equal(M, first[t][1]), t
            first.setdefault(t, (V, M))
        assert all(v > 0.0 for v in g.cluster_ms())


@pytest.mark.parametrize("pat", ("interleaved", "sorted"))
def test_local_communicator_ranks_agree(big, pat):
    X, y, f, cond, pats = big
    ids, G, one = pats[pat]
    comm = D.LocalComm(2)
    res, errs = {}, []

    def run(r):
        try:
            lo, hi = D.shard_range(N_BIG, 2, r)
            with Engine(0) as e:
                e.set_comm_local(comm.rank(r))
                e.set_data(np.asfortranarray(X[lo:hi]), y[lo:hi])
                e.set_clusters(ids[lo:hi], G)  # global codes
                res[r] = {t: e.vcov_cluster(f.coefs, "binomial", "logit", type=t, return_meat=True)
                          for t in ("HC0", "HC1")}
                for t in ("HC0", "HC1"):  # again: the all-reduced S of the last call is not summed in
                    again = e.vcov_cluster(f.coefs, "binomial", "logit", type=t, return_meat=True)
                    assert np.array_equal(again[0], res[r][t][0]) and np.array_equal(again[1], res[r][t][1]), t
                # ranks that declare different G are refused on every rank, before the large all-reduce
                e.set_clusters(ids[lo:hi], G + r)
                with pytest.raises(L.IllegalArgumentException, match="same number of clusters"):
                    e.vcov_cluster(f.coefs, "binomial", "logit")
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    comm.close()
    assert not errs, errs
    for t in ("HC0", "HC1"):
        for k in (0, 1):
            assert np.array_equal(res[0][t][k], res[1][t][k]), t
        assert scaled_err(res[0][t][1], one[(t, True)][1]) <= 1e-9, t
        assert scaled_err(res[0][t][0], one[(t, True)][0]) <= v_bar(cond), t


def test_an_id_without_rows_counts_in_G(eng):
    n, p = 2 * T + 1000, 17
    X, y, beta, cond = logit(eng, n, p)
    ids, G = CR.make_ids("two_level", n, T)
    a = check("empty id", eng, X, y, beta, "binomial", "logit", cond, ids, G + 1, cadjusts=(True, False))
    b = check("no empty id", eng, X, y, beta, "binomial", "logit", cond, ids, G, cadjusts=(True, False))
    assert np.array_equal(a[("HC0", False)][1], b[("HC0", False)][1])  # the meat: a zero row of S adds nothing
    assert np.array_equal(a[("HC0", False)][0], b[("HC0", False)][0])
    assert not np.array_equal(a[("HC0", True)][0], b[("HC0", True)][0])  # G / (G - 1) differs


def test_refusals(eng):
    lib = L.load()
    n, p = 1000, 6
    X, y, _, _ = synth.generate(0, 0, n, p, 3)
    ids = np.arange(n) % 7
    beta = np.zeros(p)
    with Engine(0) as fresh:
        with pytest.raises(L.IllegalArgumentException, match="no data set"):
            fresh.set_clusters(ids, 7)  # before any data
    eng.set_data(X, y)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.vcov_cluster(beta, "binomial", "logit")  # no clusters set
    eng.set_clusters(ids, 7)
    eng.set_data(X, y)  # replaces the data: the clusters are dropped
    with pytest.raises(L.IllegalArgumentException, match="sglm_set_clusters"):
        eng.vcov_cluster(beta, "binomial", "logit")
    with pytest.raises(L.IllegalArgumentException, match="resident rows"):
        eng.set_clusters(ids[:-1], 7)  # wrong length
    bad = np.ascontiguousarray(ids, dtype=np.int32)
    for G in (6, 0):  # id >= G, straight at the C ABI
        assert lib.sglm_set_clusters(eng._h, bad.ctypes.data_as(C.POINTER(C.c_int32)), n, G) == L.SGLM_EINVAL
    with pytest.raises(L.IllegalArgumentException, match=r"\[0, G = 6\)"):
        eng.set_clusters(ids, 6)
    eng.set_clusters(ids, 7)
    o = L.GlmOpts(0, 0, 1e-6, 0, 0, 0, 0)
    cov = np.zeros((p, p), order="F")
    for hc in (2, 3):  # HC2 / HC3
        assert lib.sglm_vcov_cluster(eng._h, C.byref(o), L.ptr(beta), hc, 1, cov.ctypes.data_as(L.dp),
                                     None) == L.SGLM_EINVAL
    eng.set_clusters(np.zeros(n, dtype=np.int64), 1)
    with pytest.raises(L.IllegalArgumentException, match="G >= 2"):
        eng.vcov_cluster(beta, "binomial", "logit", cadjust=True)  # cadjust with G = 1
    assert eng.stats()["passes"] == 0  # all refused before any launch

    X2, y2, _, _ = synth.generate(0, 0, 1000, 257, 3)
    eng.set_data(X2, y2)
    eng.set_clusters(ids, 7)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="p <= 256"):
        eng.vcov_cluster(np.zeros(257), "binomial", "logit")
    assert eng.stats()["passes"] == 0
    eng.synth(0, 0, 4096, 64, 5, procedural=True)
    eng.set_clusters(np.arange(4096) % 7, 7)
    eng.reset_stats()
    with pytest.raises(L.IllegalArgumentException, match="procedural"):
        eng.vcov_cluster(np.zeros(64), "binomial", "logit")
    assert eng.stats()["passes"] == 0
    old = os.environ.get("SGLM_FORCE_WIDE")
    os.environ["SGLM_FORCE_WIDE"] = "1"
    try:
        with Engine(0) as w:
            w.set_data(X, y)
            w.set_clusters(ids, 7)
            w.reset_stats()
            with pytest.raises(L.IllegalArgumentException, match="SGLM_FORCE_WIDE"):
                w.vcov_cluster(beta, "binomial", "logit")
            assert w.stats()["passes"] == 0
    finally:
        if old is None:
            del os.environ["SGLM_FORCE_WIDE"]
        else:
            os.environ["SGLM_FORCE_WIDE"] = old
