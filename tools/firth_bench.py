"""firth_ms of the Firth kernel (influence.hip firth_kernel, past ten column blocks with firth_xtv_kernel) against
influence_ms of the per-row diagnostics kernel and pass_kernel_ms of one IRLS pass of the same shard, same box, same
run.  The yardstick is what the same job costs without the kernel: one influence call for the leverages plus one
further read of X for X'v -- at least influence_ms + the stream time of X.

Synthetic logit designs generated in HBM (sglm_synth): 100M x 32, 20M x 64, 20M x 128, 20M x 256 by default;
SHAPES="n,p n,p ..." selects others.  Per shape: WARM untimed rounds, then REPS rounds of (one IRLS pass, one
influence call, one Firth pass), alternating; the medians (HIP events), the ratios, the route the width takes and the
kernel's HBM rate from the bytes the route reads (8 p + 8 + 24 per row fused; the two-kernel route writes and reads v
and reads X again).  One JSON line per shape, appended to OUT (default profiles/firth_bench.jsonl).

    python tools/firth_bench.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkglm_amd import Engine  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"
HBM_PEAK = 8.0e12  # bytes / s
FUSED_MAX_P16 = 10  # influence.hip FIRTH_FUSED_MAX


def run(eng, n, p, warm, reps):
    eng.synth(0, 0, n, p, 2)
    beta = np.full(p, 0.01)
    firth, infl, pas = [], [], []
    for k in range(warm + reps):
        eng.reset_stats()
        eng.irls_pass(beta)
        s = eng.stats()
        eng.influence(beta, "binomial", "logit")
        eng.firth_pass(beta, "binomial", "logit")
        if k >= warm:
            pas.append(s["pass_kernel_ms"])
            infl.append(eng.influence_ms())
            firth.append(eng.firth_ms())
    P16 = (p + 15) // 16
    fused = P16 <= FUSED_MAX_P16
    f_ms, i_ms, p_ms = float(np.median(firth)), float(np.median(infl)), float(np.median(pas))
    stream_ms = n * 8.0 * p / HBM_PEAK * 1e3
    hbm = n * (8.0 * p + 8.0 + 24.0) if fused else n * (16.0 * p + 8.0 + 24.0 + 16.0)
    return {
        "n": n, "p": p, "P16": P16, "reps": reps, "route": "fused" if fused else "rows + xtv",
        "firth_ms": f_ms, "influence_ms": i_ms, "pass_kernel_ms": p_ms, "firth_over_influence": f_ms / i_ms,
        "firth_over_pass": f_ms / p_ms, "stream_ms_at_peak": stream_ms,
        "firth_over_influence_plus_stream": f_ms / (i_ms + stream_ms),
        "firth_ms_min": float(min(firth)), "firth_ms_max": float(max(firth)),
        "influence_ms_min": float(min(infl)), "influence_ms_max": float(max(infl)),
        "pass_kernel": s["pass_kernel_name"], "hbm_TBps": hbm / (f_ms * 1e-3) / 1e12,
    }


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", DEFAULT).split()]
    warm, reps = int(os.environ.get("WARM", "2")), int(os.environ.get("REPS", "7"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "firth_bench.jsonl"))
    with Engine(0) as eng:
        for n, p in shapes:
            line = json.dumps(run(eng, n, p, warm, reps))
            print(line, flush=True)
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
