#!/bin/bash
# tests + full bench + rocprof kernel stats (each step time-limited; a crash or
# timeout stops the script, test failures do not); profile under $PROF_OUT
export PROF_OUT=${PROF_OUT:-bench_out/prof}
exec tools/gpu_steps.sh \
  "1000|gpu_tests|python -u -m pytest tests -m gpu -q -rf --timeout 240 --timeout-method thread" \
  "300|bench|python -u bench.py --full --steps 60 --warmup 5" \
  "240|prof|rocprofv3 --kernel-trace --stats -d \$PROF_OUT -o run --output-format csv -- python3 bench.py --full --steps 40 --warmup 5 --no-cpu-baseline"
