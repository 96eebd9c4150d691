"""influence_ms of the per-row diagnostics kernel (influence.hip) against pass_kernel_ms of one IRLS
pass of the same shard, same box, same run -- the pass is the yardstick: the same HBM bytes (plus
up to 24 B / row of outputs here) and the same fp64 MFMA flops.

Synthetic logit designs generated in HBM (sglm_synth): 100M x 32, 20M x 64, 20M x 128, 20M x 256 by
default; SHAPES="n,p n,p ..." selects others.  Per shape: WARM untimed rounds, then REPS rounds of
(one IRLS pass, one influence call with every output), the two alternating; the medians, the
ratio, the kernel's HBM rate and fp64 MFMA rate from the bytes and flops the shape needs
(8 p + 8 bytes read and 24 written per row; 2 * 256 * T * 16 flops per 16 rows, T = P16 (P16 + 1) / 2
tiles) and C~'s L2 traffic per row.  One JSON line per shape; OUT=file appends them there.

    python tools/influence_bench.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkglm_amd import Engine  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"
HBM_PEAK, MFMA_PEAK = 8.0e12, 78.6e12  # bytes / s, fp64 MFMA flop / s


def run(eng, n, p, warm, reps):
    eng.synth(0, 0, n, p, 2)
    beta = np.full(p, 0.01)
    infl, pas = [], []
    for k in range(warm + reps):
        eng.reset_stats()
        eng.irls_pass(beta)
        s = eng.stats()
        eng.influence(beta, "binomial", "logit")
        if k >= warm:
            pas.append(s["pass_kernel_ms"])
            infl.append(eng.influence_ms())
    P16 = (p + 15) // 16
    T = P16 * (P16 + 1) // 2
    rows_per_step = 128 if P16 <= 7 else 64
    i_ms, p_ms = float(np.median(infl)), float(np.median(pas))
    hbm = n * (8.0 * p + 8.0 + 24.0)
    flops = n / 16.0 * T * 4 * 2048.0
    return {
        "n": n, "p": p, "P16": P16, "reps": reps, "influence_ms": i_ms, "pass_kernel_ms": p_ms,
        "ratio": i_ms / p_ms, "influence_ms_min": float(min(infl)), "influence_ms_max": float(max(infl)),
        "pass_kernel": s["pass_kernel_name"], "hbm_TBps": hbm / (i_ms * 1e-3) / 1e12,
        "mfma_TFLOPs": flops / (i_ms * 1e-3) / 1e12,
        "bound_ms": max(hbm / HBM_PEAK, flops / MFMA_PEAK) * 1e3,
        "bound": "hbm" if hbm / HBM_PEAK >= flops / MFMA_PEAK else "mfma",
        "l2_bytes_per_row": T * 2048.0 / rows_per_step, "l2_over_hbm": T * 2048.0 / rows_per_step / (8.0 * p),
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
