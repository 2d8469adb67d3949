#!/bin/bash
# A/B of entropy phase timers and bench lines: VARIANTS="nobb ..." bash tools/ab_phases.sh
# (logs under $OUT)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for v in $VARIANTS; do
  SPDL_AMD_LIB=spdl_amd/lib/variants/libspdl_hipjpeg_$v.so timeout -k 10 150 python tools/debug/phases.py > $OUT/ph_$v.log 2>&1 || { tail -5 $OUT/ph_$v.log; exit 1; }
  echo "variant $v"; cat $OUT/ph_$v.log
  for l in 4 1; do
    SPDL_AMD_LIB=spdl_amd/lib/variants/libspdl_hipjpeg_$v.so timeout -k 10 150 python -u bench.py --full --steps 200 --warmup 10 --no-cpu-baseline --no-queue-compare --lanes1-steps 0 --lanes $l > $OUT/b_${v}_l$l.log 2>&1 || { tail -5 $OUT/b_${v}_l$l.log; exit 1; }
    python -c "
import json
for l in open('$OUT/b_${v}_l$l.log'):
    if l.startswith('{\"metric'):
        d=json.loads(l); print('  lanes $l', d['value'], {k: round(v,3) for k,v in d['stages_ms'].items()})"
  done
done
