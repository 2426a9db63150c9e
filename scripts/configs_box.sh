#!/bin/bash
# GPU box: bench lines (with CPU baseline + oracle prefix parity) of the non-headline configs C2, C4, C5.
# Usage: bash scripts/configs_box.sh <tag>
set -o pipefail
OUT_DIR=${KYV_OUT_DIR:-bench_out}  # where the logs go (relative to the repository root)
TAG=${1:-cfg}
mkdir -p $OUT_DIR
for w in c2 c5 c4; do
  S=20; [ $w = c4 ] && S=3
  timeout -k 10 400 python -u bench.py --full --workload $w --steps $S --warmup 1 --no-e2e > $OUT_DIR/${TAG}_$w.log 2>&1 || { echo "FAIL $w"; tail -20 $OUT_DIR/${TAG}_$w.log; exit 1; }
  python -c "import json; d=json.loads([l for l in open('$OUT_DIR/${TAG}_$w.log') if l.startswith('{')][0]); print('$w', '%.4g evals/s' % d['value'], '%.3f ms/step' % d['ms_per_step'], 'cpu %.4g' % d['cpu_baseline']['value'], 'parity', d['parity_prefix']['status'], d['parity_prefix']['pairs_compared'], 'fb', d['config']['cpu_fallback_pairs_per_step'])"
done
