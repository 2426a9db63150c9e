#!/bin/bash
# GPU box: parity tests then a short bench (no CPU baseline). Usage: bash scripts/gpu_check.sh <tag> [bench args]
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-chk}; shift
mkdir -p $OUT_DIR
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_tests.log; exit 1; }
tail -3 $OUT_DIR/${TAG}_tests.log
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 2 --no-cpu-baseline "$@" > $OUT_DIR/${TAG}_bench.log 2>&1 || { tail -30 $OUT_DIR/${TAG}_bench.log; exit 2; }
grep -v "^{" $OUT_DIR/${TAG}_bench.log | tail -5
python -c "import json,sys; d=json.loads([l for l in open('$OUT_DIR/${TAG}_bench.log') if l.startswith('{')][0]); print('VALUE %.4g evals/s  kernel %.3f ms  frac %.4f' % (d['value'], d['roofline']['kernel_ms'], d['roofline']['frac']))"
