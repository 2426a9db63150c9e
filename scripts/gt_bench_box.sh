#!/bin/bash
# GPU box: selected GPU tests, then a short default bench (timed line + native gather, no CPU baseline / e2e).
# Usage: bash scripts/gt_bench_box.sh <tag> <pytest -k expression>
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=$1
mkdir -p $OUT_DIR
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread -k "$2" > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -40 $OUT_DIR/${TAG}_tests.log; exit 1; }
tail -2 $OUT_DIR/${TAG}_tests.log
timeout -k 10 400 python -u bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-e2e --no-account > $OUT_DIR/${TAG}_bench.log 2>&1 || { tail -20 $OUT_DIR/${TAG}_bench.log; exit 2; }
grep -v "^{" $OUT_DIR/${TAG}_bench.log | tail -4
