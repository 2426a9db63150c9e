#!/bin/bash
# GPU box: GPU tests, then C2 new-vs-alt library A/B, then C5 with / without the deny kernel.
# Usage: bash scripts/combo_box.sh <tag> <alt lib>
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=$1
mkdir -p $OUT_DIR/ab
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT_DIR/${TAG}_tests.log 2>&1 || { tail -40 $OUT_DIR/${TAG}_tests.log; exit 1; }
tail -2 $OUT_DIR/${TAG}_tests.log
bash scripts/c2_ab_box.sh $2 || exit 2
export KYV_CORPUS_CACHE=/tmp/kc5
for n in d1 d0 d1b; do
  if [ $n = d0 ]; then E="KYV_DENY_KERNEL=0"; else E="KYV_X=0"; fi
  env $E timeout -k 10 300 python -u bench.py --full --workload c5 --steps 10 --warmup 2 --no-cpu-baseline --no-e2e --no-account > $OUT_DIR/ab/c5_$n.log 2>&1 || { echo "FAIL $n"; tail -5 $OUT_DIR/ab/c5_$n.log; exit 3; }
  python -c "import json; d=json.loads([l for l in open('$OUT_DIR/ab/c5_$n.log') if l.startswith('{')][0]); print('c5 %-4s eval %.4f ms value %.4g phases %s' % ('$n', d['roofline']['evaluation_ms'], d['value'], {k: round(x, 4) for k, x in d['roofline']['phase_ms'].items()}))"
done
