#!/usr/bin/env bash
# GPU-box script: GPU tests, the full bench line, the rocprofv3 kernel-stats run of the same bench and the two
# HBM PMC passes (FETCH_SIZE / WRITE_SIZE in separate runs, timed steps only). Everything lands in $OUT (default
# refresh_out/, ignored by git); summarise with
#   tools/prof_summary.py $OUT/prof/run_results.db --csv profiles/rNN_kernel_stats_cfg2.csv
#   tools/pmc_summary.py --fetch $OUT/pmc_fetch --write $OUT/pmc_write --config cfg2 --out profiles/pmc_cfg2.json
# Each GPU step has its own time limit; the script stops at the first failing step.
set -euo pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp PYTHONUNBUFFERED=1
OUT=${FWAV_REFRESH_OUT:-refresh_out}
mkdir -p "$OUT"
step() {  # name seconds command...
  local name=$1 secs=$2
  shift 2
  echo "=== $name"
  timeout -k 10 "$secs" "$@" > "$OUT/$name.log" 2>&1 || { echo "step $name failed: $?"; tail -20 "$OUT/$name.log"; exit 1; }
  tail -3 "$OUT/$name.log"
}
step gputests 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread
step bench 600 python -u bench.py --full
rm -rf "$OUT/prof" "$OUT/pmc_fetch" "$OUT/pmc_write"
step prof 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 bench.py --full --no-cpu-baseline
step pmc_fetch 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_fetch" -- python3 bench.py --steps 2 --warmup 1
step pmc_write 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_write" -- python3 bench.py --steps 2 --warmup 1
find "$OUT/prof" -name "*.db" | head -3
