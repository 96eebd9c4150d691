"""One GEE iteration (sglm_gee_pass: the pass that stores eta, gee_rows_kernel, the segment sums of sqrt(w) x,
the combine, the moments, the Gram pass over the scaled group sums) beside one fixed-effects iteration
(sglm_fe_pass) on the same handle, the same ids, the same run.  The two steps read the same bytes and differ by
two scalar columns per segment and group, so the yardstick of the GEE step is the FE step measured here; the
spread between the repeated FE steps of the run is printed beside the gap.

The shapes and id layouts of tools/fe_bench.py (synthetic logit designs generated in HBM; SHAPES="n,p ..."
selects others).  Per case: WARM untimed rounds, then REPS rounds of (fe_pass, gee_pass), alternating; HIP-event
kernel times (the pass, rows / weights, segment sums, combine, Gram), medians and min / max; ORDER=gee,fe runs the
GEE step of every round first (an A/B of the order).  rho is fixed at 0.2
so that every round runs the same downdate.  One JSON line per case; OUT=file appends them there
(profiles/gee_bench.jsonl).

    OUT=profiles/gee_bench.jsonl python tools/gee_bench.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine, _lib as L  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"
PARTS = ("pass", "rows", "sum", "combine", "gram")


def run(eng, n, p, label, ids, G, warm, reps):
    beta, alpha = np.full(p, 0.01), np.full(G, 0.02)
    eng.set_clusters(ids, G)
    nseg = len(L.cluster_plan(ids, G)[1]) - 1
    t = {s + "_" + k: [] for s in ("fe", "gee") for k in PARTS}
    gee_first = os.environ.get("ORDER", "fe,gee") == "gee,fe"  # which step of a round runs first

    def fe_step():
        eng.fe_pass(beta, alpha, "binomial", "logit", sums=False)
        return (eng.stats()["last_pass_ms"],) + eng.fe_ms()

    def gee_step():
        eng.gee_pass(beta, "binomial", "logit", rho=0.2, sums=False)
        return (eng.stats()["last_pass_ms"],) + eng.gee_ms()

    for k in range(warm + reps):
        if gee_first:
            gee, fe = gee_step(), fe_step()
        else:
            fe, gee = fe_step(), gee_step()
        if k >= warm:
            for key, a, b in zip(PARTS, fe, gee):
                t["fe_" + key].append(a)
                t["gee_" + key].append(b)
    out = {"n": n, "p": p, "clusters": label, "G": G, "nseg": nseg, "reps": reps, "order": "gee,fe" if gee_first else "fe,gee"}
    for k, v in t.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_ms_range"] = [float(min(v)), float(max(v))]
    for s in ("fe", "gee"):
        tot = [sum(t[s + "_" + k][r] for k in PARTS) for r in range(reps)]
        out[s + "_step_ms"], out[s + "_step_ms_range"] = float(np.median(tot)), [min(tot), max(tot)]
    out["gee_over_fe"] = out["gee_step_ms"] / out["fe_step_ms"]
    lo, hi = out["fe_step_ms_range"]
    out["fe_spread"] = (hi - lo) / out["fe_step_ms"]  # the gap is judged against this
    n_pad = (n + 31) // 32 * 32
    out["rows_gbps"] = 8.0 * (4 * n_pad + 4 * nseg) / (out["gee_rows_ms"] * 1e-3) / 1e9  # y, eta, prior read; d written
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
