#!/bin/bash
# One GPU session: parity tests; then, only if they ran without a fault, one bench
# line per config and a rocprofv3 kernel-trace summary of the default bench.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
timeout -k 10 ${PYTEST_TIMEOUT:-900} python -m pytest tests -m gpu -q -rf ${PYTEST_ARGS:-} > $O/pytest_gpu.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -15 $O/pytest_gpu.log
[ $rc -le 1 ] || exit $rc
for cfg in ${BENCH_CONFIGS:-deit_base}; do
  timeout -k 10 ${BENCH_TIMEOUT:-600} python bench.py --full --config $cfg ${BENCH_ARGS:-} > $O/bench_$cfg.json 2> $O/bench_$cfg.err
  brc=$?
  echo "bench $cfg rc=$brc"; cat $O/bench_$cfg.json; tail -3 $O/bench_$cfg.err
  [ $brc -eq 0 ] || exit $brc
done
if [ -n "${PROFILE:-}" ]; then
  rm -rf $O/prof
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- \
      python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-parity ${PROFILE_ARGS:-} > $O/prof_bench.json 2> $O/prof.err
  prc=$?
  echo "rocprof rc=$prc"; find $O/prof -name "*stats*" | head
  for f in $(find $O/prof -name "*kernel_stats.csv"); do cut -c1-220 $f | head -12; done
fi
