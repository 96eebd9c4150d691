"""score_ms and meat_ms of the sandwich covariance (sglm_vcov_robust: the score-weight kernel of
influence.hip, then a Gram pass weighted by its output) against the kernels it is composed of, on the
same shard, same box, same run: meat_ms against pass_kernel_ms of one logit IRLS pass (the same kernel
family with a cheaper row stage), score_ms of HC3 against influence_ms (the same kernel, one store stream
instead of three), score_ms of HC0 for what skipping the MFMA product saves.

Synthetic logit designs generated in HBM (sglm_synth): 100M x 32, 20M x 64, 20M x 128, 20M x 256 by
default; SHAPES="n,p n,p ..." selects others.  Per shape: WARM untimed rounds, then REPS rounds of (one
IRLS pass, one influence call, one vcov_robust("HC0"), one vcov_robust("HC3")), alternating; medians
and min / max, the ratios, and `sum_ratio` = (score_ms + meat_ms of HC3) / (influence_ms +
pass_kernel_ms) -- above 1.1 the composition costs more than its parts.  One JSON line per shape;
OUT=file appends them there.

    python tools/sandwich_bench.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"


def run(eng, n, p, warm, reps):
    eng.synth(0, 0, n, p, 2)
    beta = np.full(p, 0.01)
    t = {k: [] for k in ("pass", "infl", "score0", "meat0", "score3", "meat3")}
    for k in range(warm + reps):
        eng.reset_stats()
        eng.irls_pass(beta)
        s = eng.stats()
        eng.influence(beta, "binomial", "logit")
        i_ms = eng.influence_ms()
        eng.vcov_robust(beta, "binomial", "logit", type="HC0")
        s0, m0 = eng.sandwich_ms()
        eng.vcov_robust(beta, "binomial", "logit", type="HC3")
        s3, m3 = eng.sandwich_ms()
        if k >= warm:
            for key, v in zip(t, (s["pass_kernel_ms"], i_ms, s0, m0, s3, m3)):
                t[key].append(v)
    med = {k: float(np.median(v)) for k, v in t.items()}
    rng = lambda k: [float(min(t[k])), float(max(t[k]))]
    return {
        "n": n, "p": p, "P16": (p + 15) // 16, "reps": reps, "pass_kernel": s["pass_kernel_name"],
        "pass_kernel_ms": med["pass"], "influence_ms": med["infl"],
        "score_ms_hc0": med["score0"], "meat_ms_hc0": med["meat0"],
        "score_ms_hc3": med["score3"], "meat_ms_hc3": med["meat3"],
        "pass_kernel_ms_range": rng("pass"), "influence_ms_range": rng("infl"),
        "score_ms_hc0_range": rng("score0"), "meat_ms_hc0_range": rng("meat0"),
        "score_ms_hc3_range": rng("score3"), "meat_ms_hc3_range": rng("meat3"),
        "meat_over_pass": med["meat3"] / med["pass"], "score_hc3_over_influence": med["score3"] / med["infl"],
        "score_hc0_over_hc3": med["score0"] / med["score3"],
        "sum_ratio": (med["score3"] + med["meat3"]) / (med["infl"] + med["pass"]),
        "score_share_hc3": med["score3"] / (med["score3"] + med["meat3"]),
    }


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", DEFAULT).split()]
    warm, reps = int(os.environ.get("WARM", "2")), int(os.environ.get("REPS", "7"))
    out = os.environ.get("OUT")
    with Engine(0) as eng:
        for n, p in shapes:
            line = json.dumps(run(eng, n, p, warm, reps))
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
