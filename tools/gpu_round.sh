#!/bin/bash
# GPU box routine: parity tests, then a short bench. Stops at the first crash/timeout.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-out}
mkdir -p "$OUT"
TESTS=${TESTS:-tests}
timeout -k 10 ${TEST_TIMEOUT:-900} python -m pytest $TESTS -m gpu -q -p no:cacheprovider -rs ${PYTEST_K:+-k "$PYTEST_K"} > "$OUT/gpu_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc"; tail -40 "$OUT/gpu_tests.log"
if [ $rc -gt 1 ]; then exit $rc; fi
if [ "${BENCH:-1}" = "1" ]; then
  # --full: this routine reads the ranking, test_step and cpu_baseline sections too
  timeout -k 10 ${BENCH_TIMEOUT:-400} python bench.py --full --steps ${STEPS:-30} --warmup 3 --cpu-budget ${CPU_BUDGET:-8} > "$OUT/bench.json" 2> "$OUT/bench.err"
  rc=$?
  echo "bench rc=$rc"; cat "$OUT/bench.json"; tail -5 "$OUT/bench.err"
  exit $rc
fi
