#!/bin/bash
# what the dense tail's weight stream costs the PIPELINED step (timing build -DTC_NOWLOAD, wrong results): nothing --
# 0.1804 against 0.1797 ms per step, the launch alone 52.3 against 55.2 us.  (The selection's ablation builds are for
# tools/select_variants.sh only: they change what is selected, so the kernels behind them do other work -- and the one
# without the look-back never ends.)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
run() {  # source, flags
  line=$(tools/variant.sh -t 300 -s "$1" -x "$2" -- python3 bench.py --full --gpus 1 --steps 40 --warmup 5 --rows on --launch plan --weights random --no-bf16 --no-cpu-baseline | tail -1) || exit $?
  [ -n "$line" ] || return 0   # (VARIANT_BUILD_ONLY=1: nothing ran)
  echo "[$1.hip $2] $(echo "$line" | python3 -c "
import json,sys
try:
    d=json.loads(sys.stdin.readline()); print(d['value'], d['ms_per_step'], {k:v['ms_per_step'] for k,v in list(d.get('kernels',{}).items())[:5]})
except Exception as e: print('failed', e)")"
}
run tail_chain ""
run tail_chain "-DTC_NOWLOAD"
run tail_chain ""
