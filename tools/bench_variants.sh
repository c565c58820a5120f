#!/bin/bash
# usage: [PREC=f16x3] [STEPS=30] [BENCH_ARGS="--engine-option threebody_moments=0"] tools/bench_variants.sh name1 name2 ...
# Runs bench.py once per name with lib/variants/<name>.so (tools/build_variant.sh: the kernels of another checkout, usually the
# parent commit) swapped in for the library; "base" = the built library.  Same box, same session: the comparison a change needs.
cd "$(dirname "$0")/.."
L=torch-m3gnet_amd/lib
cp $L/libm3gnet_hip.so /tmp/base.so
res=$(mktemp -d)   # each variant's bench line and log
for v in "$@"; do
  if [ "$v" = base ]; then cp /tmp/base.so $L/libm3gnet_hip.so; else cp $L/variants/$v.so $L/libm3gnet_hip.so; fi
  timeout -k 10 200 python bench.py --steps ${STEPS:-10} --warmup 3 --full --no-cpu-baseline --no-secondary --precision ${PREC:-fp32} $BENCH_ARGS > $res/bench_var_$v.json 2> $res/bench_var_$v.err || { echo "$v FAILED"; tail -3 $res/bench_var_$v.err; continue; }
  python - "$res/bench_var_$v.json" "$v" <<PY
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
s=d["config"]["stage_ms_per_step"]
print(sys.argv[2], "ms/step %.4f"%d["ms_per_step"], {k: s[k] for k in ("edge_block_fwd","edge_rev_fused","edge_rev_node_mlp","edge_rev_edge_mlp","node_rev","node_pre","threebody_rev","threebody_fwd") if k in s})
PY
done
cp /tmp/base.so $L/libm3gnet_hip.so
