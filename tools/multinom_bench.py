"""Kernel times of one multinomial Newton iteration (multinom.hip: multinom_rows_kernel, past the fused shapes with
multinom_xtr_kernel, multinom_weight_kernel; the Gram pass per block pair of the Hessian) beside influence_ms of the
per-row diagnostics kernel -- the existing kernel with the same one-read register layout -- at the same shape, same
box, same process, and beside the time to stream X once at the device-to-device copy rate this run measures.

Designs generated in HBM with torch (an intercept and N(0, 1/4) columns, class codes uniform on 0 .. K - 1) and handed
to the engine by set_data_device: 100M x 32, 20M x 64, 20M x 128, 20M x 256 by default, K = 3 and K = 8 (a shape with
(K - 1) p > 1024 is skipped); SHAPES="n,p n,p ..." and CLASSES="3 8" select others.  Per shape and K: WARM untimed
rounds, then REPS rounds of (one full evaluation with its Hessian, one deviance-only evaluation, one influence call
-- gaussian / identity: y holds class codes), the medians (HIP events).  An iteration of the fit is one Hessian, one
deviance-only trial and one full evaluation: iteration_ms is the sum of their kernel times, gram_share the Gram
passes' part of it.  One JSON line per shape and K, appended to OUT (default profiles/multinom_bench.jsonl).

    python tools/multinom_bench.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkglm_amd import Engine  # noqa: E402

DEFAULT = "100000000,32 20000000,64 20000000,128 20000000,256"


def copy_rate():
    """bytes / s moved (read + write) by a device-to-device copy of 4 GiB, the median of 5."""
    a = torch.empty(1 << 29, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * 8.0 * (1 << 29) / (float(np.median(ts[2:])) * 1e-3)


def load(eng, n, p, K):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    X = torch.empty((p, n), dtype=torch.float64, device="cuda")
    X.normal_(0.0, 0.5, generator=g)
    X[0] = 1.0
    y = torch.randint(0, K, (n,), device="cuda", generator=g).to(torch.float64)
    eng.set_data_device(X.t(), y)
    del X, y
    torch.cuda.empty_cache()


def run(eng, n, p, K, warm, reps, rate):
    load(eng, n, p, K)
    B = np.full((K - 1) * p, 0.01)
    beta = np.full(p, 0.01)
    full, xtr, wgt, gram, dev, infl = [], [], [], [], [], []
    for k in range(warm + reps):
        eng.multinom_pass(B, K)
        f = eng.multinom_ms()
        eng.multinom_pass(B, K, hessian=False)
        d = eng.multinom_ms()[0]
        eng.influence(beta, "gaussian", "identity")
        if k >= warm:
            full.append(f[0]); xtr.append(f[1]); wgt.append(f[2]); gram.append(f[3]); dev.append(d)
            infl.append(eng.influence_ms())
    med = lambda v: float(np.median(v))
    P16 = (p + 15) // 16
    fused = med(xtr) == 0.0  # the engine's own choice: X'R did not run
    stream_ms = n * 8.0 * p / rate * 1e3
    rows_ms = med(full) + med(xtr)
    it = rows_ms + med(dev) + med(wgt) + med(gram)
    return {
        "n": n, "p": p, "K": K, "P16": P16, "reps": reps, "route": "fused" if fused else "rows + xtr",
        "rows_ms": med(full), "xtr_ms": med(xtr), "rows_dev_ms": med(dev), "weight_ms": med(wgt), "gram_ms": med(gram),
        "influence_ms": med(infl), "rows_over_influence": rows_ms / med(infl),
        "copy_rate_TBps": rate / 1e12, "stream_ms_at_copy_rate": stream_ms, "rows_over_stream": rows_ms / stream_ms,
        "iteration_ms": it, "gram_share": med(gram) / it, "gram_passes": K * (K - 1) // 2,
        "rows_ms_min": float(min(full)), "rows_ms_max": float(max(full)),
        "influence_ms_min": float(min(infl)), "influence_ms_max": float(max(infl)),
    }


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", DEFAULT).split()]
    classes = [int(v) for v in os.environ.get("CLASSES", "3 8").split()]
    warm, reps = int(os.environ.get("WARM", "1")), int(os.environ.get("REPS", "5"))
    out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "multinom_bench.jsonl"))
    rate = copy_rate()
    with Engine(0) as eng:
        for n, p in shapes:
            for K in classes:
                if (K - 1) * p > 1024:
                    continue
                line = json.dumps(run(eng, n, p, K, warm, reps, rate))
                print(line, flush=True)
                with open(out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
