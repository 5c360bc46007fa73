#!/bin/bash
# The driver's round-end sequence on one GPU: smoke, the GPU suite, the default bench line
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/final_smoke.log 2>&1 || { tail -20 $O/final_smoke.log; exit 1; }
echo smoke ok
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -rf --timeout 200 --timeout-method thread > $O/final_pytest.log 2>&1
rc=$?; tail -2 $O/final_pytest.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > $O/final_bench.json 2> $O/final_bench.err
rc=$?; tail -c 400 $O/final_bench.json; exit $rc
