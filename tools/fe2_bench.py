"""One two-way fixed-effects iteration (sglm_fe2_pass: the pass with the effective offset, the one-way step's
weights kernel and segment sums for factor 1, the list sums for factor 2, the sweeps, the cross product) beside
the one-way iteration (sglm_fe_pass) on the same shard, same box, same run.  The yardsticks are measured here:
  (a) the one-way iteration of the same run;
  (b) for the factor-2 sums, segment_sum_kernel's time on the same shape (fe_ms' sum_ms): the same arithmetic on
      consecutive rows, so the difference is the price of the gather;
  (c) for a sweep, the 16 n (p + 1) bytes it gathers, as GB/s (compare tools/stream_bench.hip on the box).

K11's shapes (synthetic logit designs generated in HBM; SHAPES="n,p ..." selects others) with factor 1 sorted in
runs of 50 rows; factor 2 `cycle` with H = 50 (i mod 50: the balanced panel) and `random` with H = 10^5.  The
design keeps its intercept column: A is then singular, which a step -- no solve -- does not notice.  Per case:
WARM untimed rounds, then REPS rounds of (fe_pass, fe2_pass), alternating; HIP-event kernel times, medians and
min / max; the sweeps start from zero and run to the default tolerance.  One JSON line per case; OUT=file
appends them there.

    python tools/fe2_bench.py
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine, _lib as L  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"
KEYS = ("fe_pass", "fe_weights", "fe_sum", "fe_combine", "fe_gram", "fe2_pass", "weights", "sum1", "sum2", "sweeps",
        "cross", "fe2_wall")


def run(eng, n, p, label, ids1, G, ids2, H, warm, reps):
    beta, alpha, gamma = np.full(p, 0.01), np.full(G, 0.02), np.full(H, 0.01)
    eng.set_clusters(ids1, G)
    t0 = time.perf_counter()
    eng.set_fe2(ids2, H)
    plan_s = time.perf_counter() - t0
    t = {k: [] for k in KEYS}
    nsweeps = 0
    for k in range(warm + reps):
        eng.fe_pass(beta, alpha, "binomial", "logit", sums=False)
        one = (eng.stats()["last_pass_ms"],) + eng.fe_ms()
        t0 = time.perf_counter()
        r = eng.fe2_pass(beta, alpha, gamma, "binomial", "logit", sums=False)
        wall = (time.perf_counter() - t0) * 1e3
        nsweeps = r["sweeps"]
        vals = one + (eng.stats()["last_pass_ms"],) + eng.fe2_ms() + (wall,)
        if k >= warm:
            for key, v in zip(KEYS, vals):
                t[key].append(v)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"n": n, "p": p, "factor2": label, "G": G, "H": H, "reps": reps, "sweeps": nsweeps, "set_fe2_s": plan_s}
    for k in KEYS:
        out[k + "_ms"] = med[k]
        out[k + "_ms_range"] = [float(min(t[k])), float(max(t[k]))]
    one_total = [sum(t[k][r] for k in ("fe_pass", "fe_weights", "fe_sum", "fe_combine", "fe_gram")) for r in range(reps)]
    two_total = [sum(t[k][r] for k in ("fe2_pass", "weights", "sum1", "sum2", "sweeps", "cross")) for r in range(reps)]
    out["fe_iter_ms"], out["fe_iter_ms_range"] = float(np.median(one_total)), [min(one_total), max(one_total)]
    out["fe2_iter_ms"], out["fe2_iter_ms_range"] = float(np.median(two_total)), [min(two_total), max(two_total)]
    out["fe2_over_fe"] = out["fe2_iter_ms"] / out["fe_iter_ms"]
    out["sum2_over_segment_sum"] = med["sum2"] / med["fe_sum"]
    out["ms_per_sweep"] = med["sweeps"] / max(nsweeps, 1)
    out["sweep_gather_gbps"] = 16.0 * n * (p + 1) / (out["ms_per_sweep"] * 1e-3) / 1e9
    return out


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", DEFAULT).split()]
    warm, reps = int(os.environ.get("WARM", "1")), int(os.environ.get("REPS", "3"))
    out = os.environ.get("OUT")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")

    with Engine(0) as eng:
        for n, p in shapes:
            eng.synth(0, 0, n, p, 2)
            i = np.arange(n, dtype=np.int64)
            ids1 = (i // 50).astype(np.int32)
            G = int(ids1[-1]) + 1
            emit(run(eng, n, p, "cycle/50", ids1, G, (i % 50).astype(np.int32), 50, warm, reps))
            H = min(100_000, max(n // 10, 1))
            ids2 = np.random.default_rng(7).integers(0, H, n).astype(np.int32)
            emit(run(eng, n, p, f"random/{H}", ids1, G, ids2, H, warm, reps))


if __name__ == "__main__":
    main()
