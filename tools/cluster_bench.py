"""sum_ms, combine_ms and gram_ms of the cluster-robust covariance (sglm_vcov_cluster: the signed-score
kernel of influence.hip, the segment-sum and combine kernels of cluster.hip, a Gram pass over the cluster
sums) beside meat_ms and score_ms of vcov_robust("HC0") -- the kernels that read the same X once -- on the
same shard, same box, same run.

Synthetic logit designs generated in HBM (sglm_synth), the shapes of tools/sandwich_bench.py: 100M x 32,
20M x 64, 20M x 128, 20M x 256 by default; SHAPES="n,p n,p ..." selects others.  Per shape, rows sorted by
cluster in clusters of 50, of n / 10 and of n / 1000 rows, and `interleaved` ids (i % 37: every row its own
segment) on a shard of n / INTER_DIV rows (default 8), whose segment sums -- as large as X -- fit.  Per case:
WARM untimed rounds, then REPS rounds of (vcov_robust("HC0"), vcov_cluster("HC0")), alternating; medians
and min / max, sum_ms / meat_ms, and the segment-sum kernel's achieved GB/s over the bytes it must move
(X and u once, the segment sums once).  One JSON line per case; OUT=file appends them there.

    python tools/cluster_bench.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine, _lib as L  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"


def run(eng, n, p, label, ids, G, warm, reps):
    beta = np.full(p, 0.01)
    eng.set_clusters(ids, G)
    tile, start, _ = L.cluster_plan(ids, G)
    nseg = len(start) - 1
    t = {k: [] for k in ("score0", "meat0", "score", "sum", "combine", "gram")}
    for k in range(warm + reps):
        eng.vcov_robust(beta, "binomial", "logit", type="HC0")
        s0, m0 = eng.sandwich_ms()
        eng.vcov_cluster(beta, "binomial", "logit", type="HC0", cadjust=False)
        vals = (s0, m0) + eng.cluster_ms()
        if k >= warm:
            for key, v in zip(t, vals):
                t[key].append(v)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rng = lambda k: [float(min(t[k])), float(max(t[k]))]
    n_pad = (n + 31) // 32 * 32
    nbytes = 8.0 * (n_pad * p + n_pad + nseg * p)
    out = {"n": n, "p": p, "clusters": label, "G": G, "nseg": nseg, "tile_rows": tile, "reps": reps}
    for key, name in (("score0", "score_ms_hc0"), ("meat0", "meat_ms_hc0"), ("score", "score_ms"), ("sum", "sum_ms"),
                      ("combine", "combine_ms"), ("gram", "gram_ms")):
        out[name] = med[key]
        out[name + "_range"] = rng(key)
    out["sum_over_meat"] = med["sum"] / med["meat0"]
    out["cluster_over_meat"] = (med["sum"] + med["combine"] + med["gram"]) / med["meat0"]
    out["sum_gbps"] = nbytes / (med["sum"] * 1e-3) / 1e9
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
