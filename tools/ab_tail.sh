#!/bin/bash
# Same-box A/B of the DeiT-base main line (with its parity check) under libmxa.so and LIBS variants.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
for rep in 1 2; do for lib in default ${LIBS:-}; do
  L=""; [ $lib != default ] && L=mx_quantization_amd/libmxa_$lib.so
  MXA_LIB=$L timeout -k 10 200 python bench.py --full --no-cpu-baseline --config deit_base --lines main > $O/abt_$lib.json 2> $O/abt_$lib.err || { tail -5 $O/abt_$lib.err; exit 1; }
  python -c "import json;d=json.load(open('$O/abt_$lib.json'));print('$lib',round(d['ms_per_step'],3),{k:round(v,3) for k,v in d['stages_ms'].items()},d['parity']['idx_bitmatch'])"
done; done
