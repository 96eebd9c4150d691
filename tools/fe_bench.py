"""One fixed-effects iteration (sglm_fe_pass: the pass with the effective offset, fe_weights_kernel, the
segment sums of w x, the combine, the Gram pass over the group sums) beside a plain IRLS iteration and one
vcov_cluster call on the same shard, same box, same run -- the yardstick is the parent's own components
measured here: plain pass + sum_ms + combine_ms + gram_ms of vcov_cluster, plus the weights kernel.

The shapes and id layouts of tools/cluster_bench.py (synthetic logit designs generated in HBM; SHAPES="n,p ..."
selects others): rows sorted by cluster in clusters of 50, n / 10 and n / 1000 rows, and 37 interleaved
clusters on a shard of n / INTER_DIV rows.  The design keeps its intercept column: A is then singular, which a
step -- no solve -- does not notice.  Per case: WARM untimed rounds, then REPS rounds of (irls_iterations 1,
fe_pass, vcov_cluster), alternating; HIP-event kernel times, medians and min / max.  One JSON line per case;
OUT=file appends them there.

    python tools/fe_bench.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine, _lib as L  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"
KEYS = ("plain", "fe_pass", "weights", "sum", "combine", "gram", "cl_sum", "cl_combine", "cl_gram")


def run(eng, n, p, label, ids, G, warm, reps):
    beta, alpha = np.full(p, 0.01), np.full(G, 0.02)
    eng.set_clusters(ids, G)
    nseg = len(L.cluster_plan(ids, G)[1]) - 1
    t = {k: [] for k in KEYS}
    for k in range(warm + reps):
        eng.irls_iterations(beta, 1, "binomial", "logit")
        plain = eng.stats()["last_pass_ms"]
        eng.fe_pass(beta, alpha, "binomial", "logit", sums=False)
        fe = (eng.stats()["last_pass_ms"],) + eng.fe_ms()
        eng.vcov_cluster(beta, "binomial", "logit", type="HC0", cadjust=False)
        vals = (plain,) + fe + eng.cluster_ms()[1:]
        if k >= warm:
            for key, v in zip(KEYS, vals):
                t[key].append(v)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"n": n, "p": p, "clusters": label, "G": G, "nseg": nseg, "reps": reps}
    for k in KEYS:
        out[k + "_ms"] = med[k]
        out[k + "_ms_range"] = [float(min(t[k])), float(max(t[k]))]
    fe_total = [sum(t[k][r] for k in ("fe_pass", "weights", "sum", "combine", "gram")) for r in range(reps)]
    yard = [sum(t[k][r] for k in ("plain", "weights", "cl_sum", "cl_combine", "cl_gram")) for r in range(reps)]
    out["fe_iter_ms"], out["fe_iter_ms_range"] = float(np.median(fe_total)), [min(fe_total), max(fe_total)]
    out["yardstick_ms"], out["yardstick_ms_range"] = float(np.median(yard)), [min(yard), max(yard)]
    out["fe_over_plain"] = out["fe_iter_ms"] / med["plain"]
    out["fe_over_yardstick"] = out["fe_iter_ms"] / out["yardstick_ms"]
    n_pad = (n + 31) // 32 * 32
    out["weights_gbps"] = 8.0 * (4 * n_pad + 2 * nseg) / (med["weights"] * 1e-3) / 1e9  # y, eta, o* read; w written
    return out


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", DEFAULT).split()]
    warm, reps = int(os.environ.get("WARM", "2")), int(os.environ.get("REPS", "5"))
    div = int(os.environ.get("INTER_DIV", "8"))
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
            for label, size in (("sorted/50", 50), ("sorted/n/10", max(n // 10, 1)), ("sorted/n/1000", max(n // 1000, 1))):
                ids = (i // size).astype(np.int32)
                emit(run(eng, n, p, label, ids, int(ids[-1]) + 1, warm, reps))
            m = max(n // div, 37)
            eng.synth(0, 0, m, p, 2)
            emit(run(eng, m, p, "interleaved", (np.arange(m) % 37).astype(np.int32), 37, warm, reps))


if __name__ == "__main__":
    main()
