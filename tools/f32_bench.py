"""fp32 against fp64 storage of a narrow design, on one shard in one process (development tool).
usage: python tools/f32_bench.py [--reps R] [--iters K] [--scale S] [--out FILE]

Per shape: the design is synthesised as fp64 and K IRLS iterations are timed (sglm_irls_iterations; kernel ms
per pass from sglm_get_stats), then the same design is stored as fp32 (store_f32) and the same iterations are
timed again.  Odd repetitions take the fp32 side first (synth(storage="f32"), then a fresh fp64 synth), so that
neither side always runs on the warmer device.  Each repetition appends one line per side to FILE (default
profiles/f32_bench.jsonl) and the last line of a shape carries the medians and their ratio.  The host ingest of
20M x 32 (set_data against set_data(storage="f32") from host arrays, INGESTS calls per window after a warm-up
of each) is timed the same way.  --scale shrinks the row counts (rehearsals).  A shape that fp64 cannot hold is
not measured here: the tool builds its fp32 designs by store_f32, which needs the fp64 image first, and a host
float array of such a shape (sglm_set_data_f32 would take it) is beyond what this tool generates."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkglm_amd import Engine  # noqa: E402

SHAPES = [  # (rows, p, synth kind, family, link)
    (100_000_000, 32, 0, "binomial", "logit"),
    (20_000_000, 64, 0, "binomial", "logit"),
    (125_000_000, 64, 2, "poisson", "log"),
    (100_000_000, 16, 1, "gaussian", "identity"),
]
INGESTS = 4  # set_data calls per timed window of the ingest comparison


def timed_passes(e, p, family, link, iters):
    e.irls_iterations(np.zeros(p), 2, family=family, link=link)  # warm-up: code objects, clocks
    e.reset_stats()
    e.irls_iterations(np.zeros(p), iters, family=family, link=link)
    st = e.stats()
    return st["pass_kernel_ms"] / st["passes"], st["pass_kernel_name"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f32_bench.jsonl"))
    a = ap.parse_args()
    out = open(a.out, "a")

    def emit(**kw):
        out.write(json.dumps(kw) + "\n")
        out.flush()
        print(json.dumps(kw), flush=True)

    with Engine(0) as e:
        for n, p, kind, family, link in SHAPES:
            n = max(1000, int(n * a.scale))
            ms = {"f64": [], "f32": []}
            for r in range(a.reps):
                for side in (("f64", "f32") if r % 2 == 0 else ("f32", "f64")):
                    if side == "f64":
                        e.synth(kind, 0, n, p, 7)
                    elif r % 2 == 0:
                        e.store_f32()  # the fp64 design just timed
                    else:
                        e.synth(kind, 0, n, p, 7, storage="f32")
                    t, name = timed_passes(e, p, family, link, a.iters)
                    ms[side].append(t)
                    emit(what="pass", n=n, p=p, family=family, link=link, storage=side, rep=r, pass_ms=t, kernel=name)
            m64, m32 = float(np.median(ms["f64"])), float(np.median(ms["f32"]))
            emit(what="pass-median", n=n, p=p, family=family, link=link, f64_ms=m64, f32_ms=m32, f64_over_f32=m64 / m32,
                 f64_spread=float(np.ptp(ms["f64"]) / m64), f32_spread=float(np.ptp(ms["f32"]) / m32))
        n, p = max(1000, int(20_000_000 * a.scale)), 32
        X = np.asfortranarray(np.random.default_rng(1).uniform(-1, 1, (n, p)))
        X32, y = X.astype(np.float32), np.zeros(n)
        ts = {"f64": [], "f32": []}
        for side in ("f64", "f32"):  # warm-up: the pinned staging buffers, the allocations
            e.set_data(X32 if side == "f32" else X, y, storage=side)
        for r in range(a.reps):
            for side in (("f64", "f32") if r % 2 == 0 else ("f32", "f64")):
                t0 = time.perf_counter()
                for _ in range(INGESTS):
                    e.set_data(X32 if side == "f32" else X, y, storage=side)  # ends in a stream synchronise
                ts[side].append((time.perf_counter() - t0) / INGESTS)
                emit(what="ingest", n=n, p=p, storage=side, rep=r, seconds=ts[side][-1])
        m64, m32 = float(np.median(ts["f64"])), float(np.median(ts["f32"]))
        emit(what="ingest-median", n=n, p=p, f64_s=m64, f32_s=m32, f64_over_f32=m64 / m32,
             f64_spread=float(np.ptp(ts["f64"]) / m64), f32_spread=float(np.ptp(ts["f32"]) / m32),
             f64_GBps=8e-9 * n * p / m64, f32_GBps=4e-9 * n * p / m32)


if __name__ == "__main__":
    main()
