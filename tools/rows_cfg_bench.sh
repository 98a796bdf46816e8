#!/bin/bash
# pair_rows D = 128 launch shapes (-DPR_CFG128=G,NTH,WTL,PER_CU,NV; the list: 32 lanes per entry, one entry per step, as
# when it was written): isolated kernel time + pipelined step
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
while IFS= read -r ex; do
  for i in 1 2; do
    line=$(tools/variant.sh -t 300 -s pair_rows -x "$ex" -- python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --rows on | tail -1) || exit $?
    [ -n "$line" ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
    echo "[$ex] $(echo "$line" | python3 tools/all_configs_fmt.py | head -2 | cut -c1-60 | tr '\n' ' ')"
  done
done <<< "${VARIANTS:-$'-DPR_CFG128=32,512,1,1,1\n-DPR_CFG128=32,512,0,2,1\n-DPR_CFG128=32,768,1,1,1\n-DPR_CFG128=32,512,1,1,1 -DPR_GRID2'}"
