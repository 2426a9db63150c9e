#!/bin/bash
# GPU box: walk-kernel parity tests (runtime-compiled and interpreted walks vs the oracle) + a 1.25M C3 bench line
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
mkdir -p $OUT_DIR
timeout -k 10 600 python -u -m pytest tests/test_gpu_parity.py -m gpu -x -v --timeout 300 --timeout-method thread -k "jit or interpreter or walk_goldens or c3_synthetic or quirk or c4_rule_slices or empty" > $OUT_DIR/qw_tests.log 2>&1 || { tail -40 $OUT_DIR/qw_tests.log; exit 1; }
tail -3 $OUT_DIR/qw_tests.log
timeout -k 10 300 python -u bench.py --full --resources 1250000 --no-cpu-baseline --no-e2e --steps 10 --warmup 2 > $OUT_DIR/qw_bench.log 2>&1 || { tail -30 $OUT_DIR/qw_bench.log; exit 3; }
grep -o '"phase_ms": {[^}]*}' $OUT_DIR/qw_bench.log
