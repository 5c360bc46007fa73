#!/bin/bash
# Round-6 check 2: smoke, the whole GPU suite, then the config's lines LINES (default main,
# qkv, qkvproj) and a kernel trace of the qkvproj line.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 1; }
echo smoke ok
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -rf --timeout 120 --timeout-method thread ${PYK:+-k "$PYK"} > $O/pt.log 2>&1
rc=$?; tail -4 $O/pt.log; [ $rc -eq 0 ] || exit $rc
for c in ${CFGS:-deit_base}; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --config $c --lines ${LINES:-main,qkv,qkvproj} > $O/bb_$c.json 2> $O/bb_$c.err || { tail -5 $O/bb_$c.err; exit 1; }
  python tools/show_bench.py $O/bb_$c.json
  rm -rf $O/tq_$c
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/tq_$c -o run --output-format csv -- \
    python bench.py --full --config $c --steps 6 --warmup 2 --no-cpu-baseline --no-parity --lines qkvproj > $O/tq_$c.log 2>&1 || exit $?
  find $O/tq_$c -name "*kernel_stats.csv" -exec cut -d, -f1-4 {} \;
done
echo done
