#!/bin/bash
# Every BASELINE config as a bench workload (1 GPU), run from the repository root: one --full JSON line
# each -> $OUT/bench_<wl>.json (OUT defaults to out/), and with PROF=1 a rocprofv3 --kernel-trace --stats
# summary of the same command -> $OUT/prof_<wl>/
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
export TMPDIR=/tmp
for wl in ${WLS:-logit256 poisson64 logit512 logit512r gamma2048 logit1b lm20}; do
  steps=10; warm=2
  [[ $wl == lm20 ]] && { steps=50; warm=5; }
  [[ $wl == gamma2048 || $wl == logit512 ]] && { steps=3; warm=1; }
  [[ $wl == logit1b ]] && { steps=5; warm=1; }
  timeout -k 10 400 python bench.py --full --workload $wl --steps $steps --warmup $warm > "$OUT/bench_$wl.json" 2> "$OUT/bench_$wl.err"
  rc=$?
  echo "$wl rc=$rc"; cat "$OUT/bench_$wl.json"
  [[ $rc -ne 0 ]] && { tail -20 "$OUT/bench_$wl.err"; exit $rc; }
  if [[ -n "$PROF" ]]; then
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$wl" -o run --output-format csv -- python bench.py --full --workload $wl --steps $steps --warmup $warm --no-cpu-baseline > "$OUT/prof_bench_$wl.json" 2> "$OUT/prof_bench_$wl.err"
    rc=$?
    echo "prof $wl rc=$rc"
    [[ $rc -ne 0 ]] && { tail -20 "$OUT/prof_bench_$wl.err"; exit $rc; }
  fi
done
exit 0
