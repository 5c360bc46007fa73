#!/bin/bash
# Same-box A/B: the main bench line of each config (CFGS) under each library (LIBS: tags of
# mx_quantization_amd/libmxa_<tag>.so, "default" = libmxa.so), no parity / CPU baseline.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
O=${OUT:-bench_out}; mkdir -p $O
for rep in 1 2; do
for lib in ${LIBS:-default}; do
  L=""; [ $lib != default ] && L=mx_quantization_amd/libmxa_$lib.so
  for c in ${CFGS:-deit_base dit_xl2}; do
    MXA_LIB=$L timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-parity --config $c --lines main > $O/ab_${lib}_$c.json 2> $O/ab_${lib}_$c.err || { tail -5 $O/ab_${lib}_$c.err; exit 1; }
    python -c "import json;d=json.load(open('$O/ab_${lib}_$c.json'));print('$lib','$c',round(d['ms_per_step'],3),'ms',{k:round(v,3) for k,v in d['stages_ms'].items()})"
  done
done
done
