#!/bin/bash
# GPU box: C4 rule-slice tests and the C4 bench line (10k policies over 1M mixed resources).
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-c4}
mkdir -p $OUT_DIR
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py -m gpu -x -v -k "c4" --timeout 300 --timeout-method thread > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -40 $OUT_DIR/${TAG}_tests.log; exit 1; }
tail -4 $OUT_DIR/${TAG}_tests.log
timeout -k 10 600 python -u bench.py --full --workload c4 --steps 3 --warmup 1 --no-e2e > $OUT_DIR/${TAG}_bench.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_bench.log; exit 3; }
grep -v "^{" $OUT_DIR/${TAG}_bench.log | tail -8
