"""Measurements of the negative binomial family: one JSON line per measurement.

    python tools/negbin_bench.py pass  N P     # negbin/log pass against the Poisson/log pass (and, P > 64, the logit pass)
    python tools/negbin_bench.py theta N       # one theta_terms_kernel launch over N rows, with and without the loglik
    python tools/negbin_bench.py thetarows N   # the theta kernel on counts on both sides of 17, theta = 2 and 1e3 (SGLM_LIB: an A/B)
    python tools/negbin_bench.py fit   N P     # a whole fit_glm_nb on overdispersed counts generated on the device

Pass and theta times are kernel times from HIP events (sglm_stats / sglm_get_theta_ms); the fit's is wall time."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine  # noqa: E402


def pass_ms(e, fam, lnk, b, reps=4):
    e.irls_pass(b, family=fam, link=lnk)
    e.reset_stats()
    for _ in range(reps):
        e.irls_pass(b, family=fam, link=lnk)
    s = e.stats()
    return s["pass_kernel_ms"] / s["passes"], s["pass_kernel_name"]


def bench_pass(n, p):
    b = np.full(p, 0.01)
    out = {"what": "pass", "n": n, "p": p}
    with Engine(0) as e:
        e.synth(2, 0, n, p, 2)   # counts, offset, prior weights
        e.set_theta(2.0)
        for rep in range(2):     # alternating, the best of two
            for fam in ("poisson", "negbin"):
                ms, name = pass_ms(e, fam, "log", b)
                out[fam + "_ms"] = min(ms, out.get(fam + "_ms", ms))
                out[fam + "_kernel"] = name
    if p > 64:
        with Engine(0) as e:
            e.synth(0, 0, n, p, 2)
            out["logit_ms"], out["logit_kernel"] = pass_ms(e, "binomial", "logit", b)
        out["negbin_over_logit"] = out["negbin_ms"] / out["logit_ms"]
    out["negbin_over_poisson"] = out["negbin_ms"] / out["poisson_ms"]
    print(json.dumps(out), flush=True)


def bench_theta(n):
    with Engine(0) as e:
        e.synth(2, 0, n, 1, 2)   # one column: the kernel reads y, eta and the prior weights only
        beta = np.array([0.5])
        e.theta_terms(beta, 2.0)
        k0, t0 = e.theta_ms()
        for _ in range(3):
            e.theta_terms(beta, 2.0)   # with the log-likelihood (lgamma)
        k1, t1 = e.theta_ms()
        e.theta_ml(beta, limit=6)      # the Newton launches (no lgamma)
        k2, t2 = e.theta_ms()
    ll, nt = (t1 - t0) / (k1 - k0), (t2 - t1) / (k2 - k1)
    print(json.dumps({"what": "theta", "n": n, "bytes_per_row": 24, "loglik_launch_ms": ll, "newton_launch_ms": nt,
                      "newton_launches": k2 - k1, "loglik_tb_s": 24 * n / ll / 1e9, "newton_tb_s": 24 * n / nt / 1e9}),
          flush=True)


def bench_theta_rows(n, reps=5):
    """Kernel time per launch on rows that take both branches (integer counts below 17: the finite sums; the rest:
    the polygamma differences), at a theta below and above the differences' switch.  Run once per library
    (SGLM_LIB), alternating, for an A/B."""
    rng = np.random.default_rng(17)
    eta = rng.uniform(1.5, 3.5, n)                      # mu 4.5 .. 33
    y = rng.poisson(np.exp(eta) * rng.gamma(2.0, 0.5, n)).astype(np.float64)
    out = {"what": "theta_rows", "lib": os.environ.get("SGLM_LIB", "tree"), "n": n, "share_y_ge_17": float(np.mean(y >= 17)),
           "reps": reps}
    with Engine(0) as e:
        e.set_data(eta.reshape(-1, 1), y, prior=rng.uniform(0.5, 1.5, n))
        beta = np.ones(1)
        for theta in (2.0, 1e3):
            e.theta_terms(beta, theta)                  # warm-up
            ms = []
            for _ in range(reps):
                k0, t0 = e.theta_ms()
                e.theta_terms(beta, theta)              # the log-likelihood instantiation
                k1, t1 = e.theta_ms()
                ms.append((t1 - t0) / (k1 - k0))
            out[f"loglik_launch_ms_theta{theta:g}"] = min(ms)
            out[f"loglik_launch_ms_theta{theta:g}_range"] = [min(ms), max(ms)]
        k0, t0 = e.theta_ms()
        r = e.theta_ml(beta, limit=8)                   # the Newton instantiation, at theta.ml's own thetas
        k1, t1 = e.theta_ms()
        out.update(newton_launch_ms=(t1 - t0) / (k1 - k0), newton_launches=k1 - k0, theta_ml=r.theta)
    print(json.dumps(out), flush=True)


def bench_fit(n, p, theta_star=2.0):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    Xt = torch.empty((p, n), dtype=torch.float64, device=dev)   # column-major n x p
    Xt.uniform_(-1.0, 1.0, generator=g)
    Xt.mul_(1.0 / np.sqrt(p))
    Xt[0].fill_(1.0)
    bstar = torch.full((p,), 0.4, dtype=torch.float64, device=dev)
    bstar[0] = 1.0
    mu = torch.exp(bstar @ Xt)
    gam = torch._standard_gamma(torch.full((n,), theta_star, dtype=torch.float64, device=dev)) / theta_star
    y = torch.poisson(mu * gam)
    del mu, gam
    with Engine(0) as e:
        e.set_data_device(Xt.t(), y)
        del Xt
        torch.cuda.empty_cache()
        e.fit_glm_nb("log")            # warm-up (allocations, first launches)
        k0, t0 = e.theta_ms()
        e.reset_stats()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        r = e.fit_glm_nb("log")
        wall = time.perf_counter() - w0
        s = e.stats()
        k1, t1 = e.theta_ms()
    print(json.dumps({"what": "fit_glm_nb", "n": n, "p": p, "theta_star": theta_star, "theta": r.theta,
                      "se_theta": r.se_theta, "wall_s": wall, "outer_iter": r.outer_iter, "passes": s["passes"],
                      "dev_passes": s["dev_passes"], "pass_kernel_ms": s["pass_kernel_ms"], "theta_launches": k1 - k0,
                      "theta_kernel_ms": t1 - t0, "theta_share_of_wall": (t1 - t0) / 1e3 / wall,
                      "converged": r.converged, "kernel": s["pass_kernel_name"]}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1]
    if what == "pass":
        bench_pass(int(sys.argv[2]), int(sys.argv[3]))
    elif what == "theta":
        bench_theta(int(sys.argv[2]))
    elif what == "thetarows":
        bench_theta_rows(int(sys.argv[2]))
    else:
        bench_fit(int(sys.argv[2]), int(sys.argv[3]))
