"""Bitwise check of every row path across library builds (development tool).
usage: AB_LIBS=a.so,b.so python tools/ab_rows.py [OUTDIR]
Each library runs in its own process on the same small designs and saves every result as an array
(OUTDIR/ab_rows_<k>.npz); the arrays of every library are then compared byte for byte with the first one's.

Fits (n = 30 011; iterations, coefficients, standard errors, deviance, null deviance, Pearson, loglik):
the narrow kernel at p = 20, 40, 64, K1 at p = 128, K1r at p = 256, the wide path at p = 272 --
binomial logit (both init modes; with m; with an offset and prior weights that include zeros) and probit,
Poisson log on counts with fractional values and values >= 256 (the reference rows beside the fast path and
the tables; offset, prior weights with zeros, both init modes) and sqrt, Gamma inverse and log, negative
binomial log and sqrt at theta = 2.
Diagnostics and the steps over the cluster factor (p = 5 and 65, the two-way designs of tests/fe2_reference.py,
every family): fit_glm_fe, fit_glm_fe2, fit_glm_gee (exchangeable, rho fixed at 0.2, independence), fe_pass and
gee_pass at 0.8 beta and in the initial mode (the GEE fits stop after GEE_ITERS iterations at the latest), vcov_fe, vcov_fe2 and vcov_gee (with their meats), influence (every
residual type), vcov_robust (HC0, HC2, HC3) and vcov_cluster at the plain fit's coefficients, firth_pass with the
leverages (binomial, Poisson) and predict_new_se of 1 000 new rows against vcov.  At p = 5 also the interleaved and
shuffled id layouts of tests/fe_reference.py, and one Poisson case on a group handle of two shards on one device
(the host sum over shards, the stale mark of the group sums).
Grids at their device cap (binomial logit, n = 140 003 -- past 131 072 rows, where on 256 CUs the widest-stepping
class, P16 <= 4, reaches its cap -- at p = 5, 65, 129, 161: one width per class of the row kernel's grid rule, the
last on the two-kernel Firth route): influence, vcov_robust HC3, firth_pass with the leverages and a 5-iteration
fit_glm_firth.  N above gives fewer steps than resident workgroups at every width, so only this block sees a
wrong cap or step.
A case that raises is recorded by its message, which must then be the same in every build."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 30_011
GEE_ITERS = 25
GRID_N = 140_003
GRID_P = (5, 65, 129, 161)  # P16 = 1, 5, 9, 11


def _fit_vec(f):
    return np.concatenate([np.ravel(f.coefs), np.ravel(f.stderr),
                           [f.deviance, f.null_deviance, f.pearson, f.loglik, float(f.iter)]])


def _zeros(pw, rng):
    pw = pw.copy()
    pw[rng.random(pw.shape[0]) < 0.03] = 0.0
    return pw


def _fit_cases():
    """(name, p, family, link, init, data()) -- data() returns dict(X, y, m, offset, prior, theta)."""
    from sparkglm_amd import synth
    import links_reference as LR
    import negbin_reference as NB

    def binomial(p, with_m=False, weights=False):
        def make():
            X, y, _, _ = synth.generate(0, 0, N, p, 7)
            rng = np.random.default_rng(p)
            d = dict(X=X, y=y)
            if with_m:
                i = np.arange(N)
                d["m"] = (i % 3 + 1 + i % 2).astype(np.float64)
                d["y"] = y * (i % 3 + 1)
            if weights:
                d["offset"] = rng.uniform(-0.1, 0.1, N)
                d["prior"] = _zeros(0.5 + rng.random(N), rng)
            return d
        return make

    def poisson_counts(p):
        def make():  # tests/test_gpu_initpass.py's counts, and prior weights with zeros
            X, y, off, prior = synth.generate(2, 0, N, p, 31)
            rng = np.random.default_rng(p)
            y = y.copy()
            y[rng.random(N) < 0.05] += 0.375
            big = rng.random(N) < 0.02
            y[big] = 256.0 + np.floor(rng.random(big.sum()) * 40.0)
            return dict(X=X, y=y, offset=off, prior=_zeros(prior, rng))
        return make

    def links(fam, p):
        def make():
            X, y, off, prior = LR.make_case(fam, N, p)
            return dict(X=X, y=y, offset=off, prior=_zeros(prior, np.random.default_rng(p)))
        return make

    def gamma_inverse(p):
        def make():
            X, y, _, _ = synth.generate(3, 0, N, p, 11)
            return dict(X=X, y=y)
        return make

    def negbin(lnk, p):
        def make():
            X, y, off, prior, _ = NB.make_case(lnk, N, p, 2.0, 100 + p)
            return dict(X=X, y=y, offset=off, prior=_zeros(prior, np.random.default_rng(p)), theta=2.0)
        return make

    out = []
    for p in (20, 40, 64, 128, 256, 272):
        for init in ("single", "multiple"):
            out.append((f"binomial:logit:{p}:{init}", "binomial", "logit", init, binomial(p)))
        out.append((f"poisson:log:{p}:single", "poisson", "log", "single", poisson_counts(p)))
        out.append((f"gamma:inverse:{p}:single", "gamma", "inverse", "single", gamma_inverse(p)))
        out.append((f"negbin:log:{p}:single", "negbin", "log", "single", negbin("log", p)))
    for p in (40, 128, 256, 272):
        out.append((f"binomial:logit:{p}:m", "binomial", "logit", "multiple", binomial(p, with_m=True)))
        out.append((f"binomial:logit:{p}:weights", "binomial", "logit", "single", binomial(p, weights=True)))
        out.append((f"binomial:probit:{p}:single", "binomial", "probit", "single", binomial(p)))
        out.append((f"poisson:log:{p}:multiple", "poisson", "log", "multiple", poisson_counts(p)))
    for p in (40, 128, 272):
        out.append((f"poisson:sqrt:{p}:single", "poisson", "sqrt", "single", links("poisson", p)))
        out.append((f"gamma:log:{p}:multiple", "gamma", "log", "multiple", links("gamma", p)))
        out.append((f"negbin:sqrt:{p}:single", "negbin", "sqrt", "single", negbin("sqrt", p)))
    return out


def _guard(res, key, run):
    """run() -> {suffix: array}; an exception is recorded by its message."""
    print("RUN", key, flush=True)
    try:
        for k, v in run().items():
            res[f"{key}:{k}"] = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    except Exception as e:  # noqa: BLE001 -- the message is the result
        res[f"{key}:error"] = np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)
        print("ERROR", key, e, flush=True)


def _named(names, values):
    return dict(zip(names, values))


def _step_cases(res, e, key, fam, lnk, beta, two_way):
    """The fits, steps and covariances over the cluster factor (and the second factor) on e's resident design."""
    def fe1():
        r = e.fit_glm_fe(fam, lnk)
        return {"fit": _fit_vec(r.fit), "alpha": r.alpha, "G_eff": [r.G_eff]}

    def fe2():
        r = e.fit_glm_fe2(fam, lnk)
        return {"fit": _fit_vec(r.fit), "alpha": r.alpha, "gamma": r.gamma}

    _guard(res, key + ":fe", fe1)
    if two_way:
        _guard(res, key + ":fe2", fe2)
    G = e._G()
    b1, a1 = res.get(key + ":fe:fit", beta)[: e.p], res.get(key + ":fe:alpha", np.zeros(G))
    for cl in (True, False):
        _guard(res, f"{key}:vcov_fe:{int(cl)}", lambda: _named(
            ("V", "meat"), e.vcov_fe(b1, a1, fam, lnk, cluster=cl, return_meat=True)))
    if two_way and key + ":fe2:fit" in res:
        _guard(res, key + ":vcov_fe2", lambda: _named(("V", "meat"), e.vcov_fe2(
            res[key + ":fe2:fit"][: e.p], res[key + ":fe2:alpha"], res[key + ":fe2:gamma"], fam, lnk, return_meat=True)))
    for b, tag in ((0.8 * beta, "beta"), (None, "init")):
        _guard(res, f"{key}:fe_pass:{tag}", lambda: _named(
            ("A", "b", "S", "t", "W", "scalars"), e.fe_pass(b, None if b is None else a1, fam, lnk, sums=True)))
        _guard(res, f"{key}:gee_pass:{tag}", lambda: e.gee_pass(b, fam, lnk, sums=True))
    # (GEE_ITERS: with rho re-estimated at every step a fit of these designs need not reach the default tol)
    for tag, kw in (("exch", {}), ("rho", dict(rho=0.2)), ("ind", dict(corstr="independence"))):
        def gee():
            r = e.fit_glm_gee(fam, lnk, max_iter=GEE_ITERS, **kw)
            return {"fit": _fit_vec(r.fit), "info": [r.rho, r.phi, r.N, r.G_eff, r.n_max]}
        _guard(res, f"{key}:gee:{tag}", gee)
    bg = res.get(key + ":gee:rho:fit", beta)[: e.p]
    for rb in (True, False):
        _guard(res, f"{key}:vcov_gee:{int(rb)}", lambda: _named(
            ("V", "meat"), e.vcov_gee(bg, 0.2, fam, lnk, robust=rb, return_meat=True)))


def _firth_pass(e, beta, fam, lnk):
    r = e.firth_pass(beta, fam, lnk, hat=True)
    return {"A": r["A"], "g": r["g"], "hat": r["hat"], "scalars": [r["deviance"], r["logdet"], r["sum_hat"]]}


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    from sparkglm_amd import Engine, synth, _lib as L
    import fe_reference as FR
    import fe2_reference as F2

    res = {}
    with Engine(0) as e:
        for name, fam, lnk, init, make in _fit_cases():
            d = make()
            if "theta" in d:
                e.set_theta(d["theta"])
            e.set_data(d["X"], d["y"], m=d.get("m"), offset=d.get("offset"), prior=d.get("prior"))
            t0 = time.perf_counter()
            _guard(res, name, lambda: {"fit": _fit_vec(e.fit_glm(fam, lnk, init=init))})
            st = e.stats()
            print(f"CASE {name:32s} {st.get('pass_kernel_kind', '?'):8s} variant {st.get('kernel_variant')} "
                  f"{time.perf_counter() - t0:.3f} s", flush=True)

        T = L.cluster_plan(np.zeros(0, dtype=np.int32), 1)[0]
        for p, layout in ((5, "sorted"), (65, "sorted"), (5, "interleaved"), (5, "shuffled")):
            n = 2 * T + 1000 + 15 * (p % 7)
            ids1, G = FR.make_ids(layout, n, T)
            ids2, H = F2.make_ids2("random", ids1, G)
            for fam, lnk in (("binomial", "logit"), ("binomial", "probit"), ("poisson", "log"), ("poisson", "sqrt"),
                             ("gamma", "log"), ("gamma", "inverse"), ("gaussian", "identity"), ("negbin", "log"),
                             ("negbin", "sqrt")):
                c = F2.make_case2(fam, lnk, n, p, ids1, G, ids2, H, 2)
                key = f"diag:{fam}:{lnk}:{p}" + ("" if layout == "sorted" else ":" + layout)
                if fam == "negbin":
                    e.set_theta(2.0)
                e.set_data(c["X"], c["y"], m=c["m"], offset=c["off"], prior=c["pw"])
                e.set_clusters(ids1, G)
                e.set_fe2(ids2, H)
                plain = {}
                _guard(plain, "b", lambda: {"coefs": e.fit_glm(fam, lnk).coefs})
                beta = plain.get("b:coefs", c["beta"])
                res[key + ":beta"] = np.ascontiguousarray(beta)
                _step_cases(res, e, key, fam, lnk, beta, True)
                if layout == "sorted":
                    for rt in ("deviance", "pearson", "working", "response"):
                        def infl():
                            r = e.influence(beta, fam, lnk, resid=rt)
                            return {"hat": r.hat, "resid": r.resid, "cooks": r.cooks, "sum_hat": [r.sum_hat]}
                        _guard(res, f"{key}:influence:{rt}", infl)
                    _guard(res, key + ":vcov_robust", lambda: {"V": e.vcov_robust(beta, fam, lnk, type="HC3")})
                    for hc in ("HC0", "HC2"):
                        _guard(res, f"{key}:vcov_robust:{hc}", lambda: {"V": e.vcov_robust(beta, fam, lnk, type=hc)})
                    _guard(res, key + ":vcov_cluster", lambda: {"V": e.vcov_cluster(beta, fam, lnk, type="HC1")})
                    if fam in ("binomial", "poisson"):
                        _guard(res, key + ":firth_pass", lambda: _firth_pass(e, beta, fam, lnk))
                    Xnew = np.random.default_rng(1000 + p).standard_normal((1000, p))
                    _guard(res, key + ":predict_new_se", lambda: {"se": e.predict_new_se(Xnew, e.vcov(beta, fam, lnk))})
                print("CASE", key, flush=True)

        # grids at their device cap (GRID_N rows: more steps than resident workgroups at every width), one width
        # per class of the grid rule
        for p in GRID_P:
            X, y, _, _ = synth.generate(0, 0, GRID_N, p, 7)
            e.set_data(X, y)
            key = f"grid:binomial:logit:{p}"
            _guard(res, key, lambda: {"beta": e.fit_glm("binomial", "logit").coefs})
            beta = res.get(key + ":beta", np.zeros(p))

            def infl():
                r = e.influence(beta, "binomial", "logit")
                return {"hat": r.hat, "resid": r.resid, "cooks": r.cooks, "sum_hat": [r.sum_hat]}

            def firth_fit():
                r = e.fit_glm_firth("binomial", "logit", maxit=5)
                return {"fit": _fit_vec(r.fit), "info": [r.converged, r.halvings, r.pen_deviance, r.logdet,
                                                         r.score_inf, r.sum_hat]}
            _guard(res, key + ":influence", infl)
            _guard(res, key + ":vcov_robust", lambda: {"V": e.vcov_robust(beta, "binomial", "logit", type="HC3")})
            _guard(res, key + ":firth_pass", lambda: _firth_pass(e, beta, "binomial", "logit"))
            _guard(res, key + ":fit_glm_firth", firth_fit)
            print("CASE", key, flush=True)

    # two shards on one device: the sums over shards go through the host, and the group sums turn stale
    with Engine(devices=[0, 0]) as e:
        p, n = 5, 2 * T + 1000 + 15 * 5
        ids1, G = FR.make_ids("sorted", n, T)
        ids2, H = F2.make_ids2("random", ids1, G)
        c = F2.make_case2("poisson", "log", n, p, ids1, G, ids2, H, 2)
        e.set_data(c["X"], c["y"], m=c["m"], offset=c["off"], prior=c["pw"])
        e.set_clusters(ids1, G)
        key = "diag:poisson:log:5:group"
        _guard(res, key, lambda: {"beta": e.fit_glm("poisson", "log").coefs})
        _step_cases(res, e, key, "poisson", "log", res.get(key + ":beta", c["beta"]), False)
        _guard(res, key + ":vcov_cluster", lambda: {"V": e.vcov_cluster(res.get(key + ":beta", c["beta"]), "poisson", "log")})
        print("CASE", key, flush=True)
    np.savez(out_path, **res)


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(outdir, exist_ok=True)
    libs = [l for l in os.environ.get("AB_LIBS", "").split(",") if l]
    runs = []
    for k, lib in enumerate(libs):
        path = os.path.join(outdir, f"ab_rows_{k}.npz")
        env = dict(os.environ, SGLM_LIB=os.path.join(ROOT, lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, timeout=900)
        if out.returncode:
            print(lib, "FAILED", out.returncode, flush=True)
            sys.exit(1)
        runs.append(dict(np.load(path)))
    bad = 0
    for k, r in enumerate(runs[1:], 1):
        for key in sorted(set(runs[0]) | set(r)):
            a, b = runs[0].get(key), r.get(key)
            same = a is not None and b is not None and a.shape == b.shape and a.tobytes() == b.tobytes()
            bad += not same
            if not same or key.endswith(":error"):
                print(f"{libs[k]:40s} {key:48s} {'bitwise' if same else 'DIFFERENT'}"
                      f"{' (an error message)' if key.endswith(':error') else ''}", flush=True)
        print(f"{libs[k]}: {len(r)} arrays, {bad} differ from {libs[0]}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
