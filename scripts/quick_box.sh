#!/bin/bash
# GPU box: selected GPU parity tests, then the default bench line (no CPU baseline) and its kernel-trace stats.
# Usage: bash scripts/quick_box.sh <tag> "<pytest -k expression or empty>" [bench args...]
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-q}; K=${2:-}; shift 2
mkdir -p $OUT_DIR
if [ -n "$K" ]; then
  timeout -k 10 500 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread -k "$K" > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -40 $OUT_DIR/${TAG}_tests.log; exit 1; }
  tail -3 $OUT_DIR/${TAG}_tests.log
fi
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline --no-e2e "$@" > $OUT_DIR/${TAG}_bench.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_bench.log; exit 3; }
grep -v "^{" $OUT_DIR/${TAG}_bench.log | tail -4
cd /tmp && export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OLDPWD/$OUT_DIR/prof_$TAG -o run -- python3 $OLDPWD/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-e2e "$@" > $OLDPWD/$OUT_DIR/${TAG}_trace.log 2>&1 || exit 4
head -6 $OLDPWD/$OUT_DIR/prof_$TAG/run_kernel_stats.csv | cut -c1-160
