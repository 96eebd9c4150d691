#!/bin/bash
# Round-end rehearsal: the GPU suite + smoke, the default workload's --full bench line (headline, 1B x 32
# strong point, configs_n1), then the same --full run under rocprofv3 --kernel-trace --stats.
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
mkdir -p gpurun_out
OUT=${OUT:-out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
export OUT
bash tools/gpu_stages.sh test,bench || exit 1
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_default" -o run --output-format csv -- python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-load > "$OUT/prof_default.json" 2> "$OUT/prof_default.err" || { echo "prof failed"; tail -20 "$OUT/prof_default.err"; exit 1; }
echo prof ok
