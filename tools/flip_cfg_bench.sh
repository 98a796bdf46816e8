#!/bin/bash
# Tuning aid: pipelined bench throughput under different launch shapes of the D = 128 flip kernel
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for cfg in "-DFL_CFG128=32,512,1,1" "-DFL_CFG128=32,512,1,2" "-DFL_CFG128=32,256,1,2" "-DFL_CFG128=32,256,0,4"; do
  line=$(tools/variant.sh -t 600 -s pair_flip -x "$cfg" -- python3 bench.py --full --steps 60 --warmup 5 --no-cpu-baseline --no-bf16 | tail -1) || exit $?
  [ -n "$line" ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
  echo "[$cfg] $(echo "$line" | python3 -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"], {k:v["ms_per_step"] for k,v in d["kernels"].items()})')"
done
