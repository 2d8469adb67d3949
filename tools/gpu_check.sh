#!/bin/bash
# GPU round trip: -m gpu tests, then (unless the tests crashed the process --
# abort / segfault / timeout, exit codes other than 0/1) one full bench line.
# Usage (on the GPU box): bash tools/gpu_check.sh [pytest -k expr]  (files under $OUT)
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
K=${1:+-k "$1"}
timeout -k 10 1000 python -u -m pytest tests -m gpu -q -rf --timeout 240 --timeout-method thread $K \
  > $OUT/gpu_tests.log 2>&1
rc=$?
tail -5 $OUT/gpu_tests.log
echo "tests rc=$rc"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -u bench.py --full --steps 60 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
brc=$?
cat $OUT/bench.json
tail -3 $OUT/bench.err
echo "bench rc=$brc"
exit $rc
