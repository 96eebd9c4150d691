"""Per-phase cycle shares of K1r's waves from a stamped development build (fused.hpp StampsR).
usage: make -C sparkglm_amd/csrc variant NAME=stamps DEFS=-DSGLM_K1R_STAMPS=1   (2: + first k-step)
       SGLM_LIB=sparkglm_amd/lib_ab/stamps/libsglm_hip.so AN=20000000 AP=256 python tools/k1r_stamps.py [out.json]
One binomial/logit pass on the seeded design of tools/ab_k1r.py; the middle workgroup's waves
report the cycles they spent in each phase, printed as shares of the mean block period.
A build with -DSGLM_K1R_STAMPS=3 records the event timeline instead: when each wave of the middle
workgroup saw or made every hand-off of one block B, printed in cycles after the earliest event."""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkglm_amd import Engine, _lib

n, p = int(os.environ.get("AN", "20000000")), int(os.environ.get("AP", "256"))
lib = _lib.load()
if not hasattr(lib, "sglm_k1r_stamps"):
    sys.exit("this library was not built with -DSGLM_K1R_STAMPS")
e = Engine(0)
e.synth(0, 0, n, p, 2)
b = np.linspace(-0.02, 0.02, p)
e.irls_pass(b)
e.reset_stats()
e.irls_pass(b)
st = e.stats()
SLOTS = 16
raw = (C.c_ulonglong * (12 * SLOTS))()
if lib.sglm_k1r_stamps(raw, 12 * SLOTS) != 0:
    sys.exit("sglm_k1r_stamps failed")
s = np.array(raw, dtype=np.float64).reshape(12, SLOTS)
if hasattr(lib, "sglm_k1r_stamps_level") and lib.sglm_k1r_stamps_level() == 3:
    EVENTS = ["done(B-2) seen", "DMA issued", "landed bumped", "landed seen", "eta 1st LDS trip", "eta reduced",
              "w, wz, eta stored", "ready bumped", "ready seen", "first k-step", "last k-step", "done bumped",
              "deviance formed"]
    t = np.array(raw, dtype=np.uint64).reshape(12, SLOTS)[:, :len(EVENTS)].astype(np.int64)
    if not t.any():
        sys.exit("no events recorded (fewer than 6 blocks in the middle workgroup?)")
    t0 = t[t > 0].min()
    out = {"n": n, "p": p, "pass_ms": st["pass_kernel_ms"] / st["passes"], "events": EVENTS,
           "waves": [{"wave": wv, "role": "gram" if wv < 8 else "row",
                      "cycles": {EVENTS[i]: int(t[wv, i] - t0) for i in range(len(EVENTS)) if t[wv, i] > 0}}
                     for wv in range(12)]}
    print(f"n={n} p={p} pass {out['pass_ms']:.3f} ms; events of one block B of the middle workgroup, cycles after the first")
    print("wave      " + " ".join(f"{k[:13]:>13s}" for k in EVENTS))
    for wv in range(12):
        print(f"{wv:2d} {'gram' if wv < 8 else 'row ':4s}   " +
              " ".join(f"{t[wv, i] - t0:13d}" if t[wv, i] > 0 else " " * 12 + "-" for i in range(len(EVENTS))))
    first = lambda i, rows: min(t[w, i] for w in rows if t[w, i] > 0) - t0
    last = lambda i, rows: max(t[w, i] for w in rows) - t0
    G, R = range(8), range(8, 12)
    chain = [("done(B-2) seen, last issuer", last(0, range(4))), ("DMA issued, last", last(1, range(4))),
             ("landed bumped, last", last(2, range(4))), ("landed seen, last row wave", last(3, R)),
             ("w stored, last row wave", last(6, R)), ("ready bumped, last row wave", last(7, R)),
             ("ready seen, first / last Gram wave", (int(first(8, G)), int(last(8, G)))), ("last k-step, last Gram wave", last(10, G)),
             ("done bumped, last wave", last(11, range(12)))]
    out["chain"] = {k: (list(map(int, v)) if isinstance(v, tuple) else int(v)) for k, v in chain}
    for k, v in chain:
        print(f"  {k:38s} {v}")
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)
    sys.exit(0)
ROW = ["wait_landed", "flag_round_or_deferred_dev", "row_stage", "wait_ready_tail", "xz_rows", "wait_done", "dma_issue"]
GRAM = ["wait_ready", "ksteps_rest", "kstep_first", "eta_done", None, None, None, None, "wait_done", "dma_issue",
        "wait_landed"]  # (the last three: Gram waves 0..3 at 16 column blocks, which issue the DMA)
out = {"n": n, "p": p, "pass_ms": st["pass_kernel_ms"] / st["passes"], "waves": []}
print(f"n={n} p={p} pass {out['pass_ms']:.3f} ms; cycles per block and share of the wave's block period")
for wv in range(12):
    names = GRAM if wv < 8 else ROW
    nb = max(s[wv, SLOTS - 1], 1.0)
    per = {k: s[wv, i] / nb for i, k in enumerate(names) if k}
    period = sum(per.values())
    out["waves"].append({"wave": wv, "role": "gram" if wv < 8 else "row", "blocks": int(nb), "period": period,
                         "cycles": per})
    hist = {"wait_ready": s[wv, 4:8]} if wv < 8 else {"wait_landed": s[wv, 7:11], "flag_round": s[wv, 11:15]}
    out["waves"][-1]["laps_le_1k_4k_16k_more"] = {k: [int(x) for x in v] for k, v in hist.items()}
    print(f"wave {wv:2d} {'gram' if wv < 8 else 'row ':4s} blocks {int(nb):5d} period {period:8.0f}  " +
          "  ".join(f"{k} {v:7.0f} ({100 * v / max(period, 1):4.1f}%)" for k, v in per.items()) +
          "  | laps <=1K/4K/16K/more: " + "  ".join(f"{k} {'/'.join(str(int(x)) for x in v)}" for k, v in hist.items()))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
