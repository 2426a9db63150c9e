#!/bin/bash
# GPU box: full GPU test suite, the default bench line (with CPU baseline), the admission micro-batching bench.
# Usage: bash scripts/final_box.sh <tag>
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-final}
mkdir -p $OUT_DIR
timeout -k 10 420 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_tests.log; exit 1; }
tail -2 $OUT_DIR/${TAG}_tests.log
timeout -k 10 400 python -u bench.py --full > $OUT_DIR/${TAG}_bench.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_bench.log; exit 2; }
grep -v "^{" $OUT_DIR/${TAG}_bench.log | tail -4
timeout -k 10 200 python -u scripts/bench_admission.py --seconds 6 > $OUT_DIR/${TAG}_admission.log 2>&1 || { tail -20 $OUT_DIR/${TAG}_admission.log; exit 3; }
grep admission $OUT_DIR/${TAG}_admission.log
