#!/bin/bash
# GPU parity suite (optional -k filter in PYK) then one bench line per config in CFGS.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
if [ -z "${NOTEST:-}" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread ${PYK:+-k "$PYK"} > $O/pt.log 2>&1
  rc=$?; tail -3 $O/pt.log; [ $rc -eq 0 ] || exit $rc
fi
for c in ${CFGS:-deit_base dit_xl2 pixart_cross}; do
  timeout -k 10 300 python bench.py --full --config $c ${BARGS:---no-cpu-baseline} > $O/b_$c.json 2> $O/b_$c.err || exit 1
done
echo ok
