#!/bin/bash
# GPU box: per-rule walk kernel times (KYV_JIT_GROUP=1: one kernel per compiled pattern rule) from a rocprofv3 kernel trace.
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
mkdir -p $OUT_DIR/split
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
KYV_JIT_GROUP=1 KYV_JIT_DEFS="-DKYV_JIT_NOEXTRA -DKYV_JIT_WPE=8" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT_DIR/split -o run -- python3 $R/bench.py --full --resources 1250000 --steps 3 --warmup 1 --no-cpu-baseline --no-e2e > $R/$OUT_DIR/split/bench.log 2>&1 || { tail -20 $R/$OUT_DIR/split/bench.log; exit 1; }
echo done
