#!/bin/bash
# GPU box: kernel-trace stats of a short bench run. Usage: bash scripts/trace_box.sh <tag> [bench args]
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-t}; shift
R=$PWD
mkdir -p $R/$OUT_DIR/trace_$TAG
cd /tmp && export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT_DIR/trace_$TAG -o run -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline "$@" > $R/$OUT_DIR/trace_$TAG/log.txt 2>&1 || exit 1
cat $R/$OUT_DIR/trace_$TAG/run_kernel_stats.csv | cut -c1-160
