#!/bin/bash
# A/B of pair_rows / tail build variants in one session, under the pipelined bench (driver form + kernel timing), with
# SERIAL=1 also the serial kernel times.  Usage: tools/variant_ab.sh  ($VARIANTS: one flag string per line, "" = the
# default build; $SOURCES: the sources those flags are for, default "pair_rows tail_chain"; $BENCH_ARGS: more bench flags)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
BARGS="--full --gpus 1 --steps 20 --warmup 5 --weights random --no-cpu-baseline --no-bf16 --rows on ${BENCH_ARGS:-}"
SOURCES=${SOURCES:-pair_rows tail_chain}
while IFS= read -r ex; do
  for i in 1 2; do
    line=$(tools/variant.sh -t 300 -s "$SOURCES" -x "$ex" -- python3 bench.py $BARGS | tail -1) || exit $?
    [ -n "$line" ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
    echo "[$ex] $(echo "$line" | python3 -c "
import json,sys
d=json.loads(sys.stdin.readline()); c=d['config']
k={a:b['ms_per_step'] for a,b in list(d.get('kernels',{}).items())[:5]}
print(d['value'], d['ms_per_step'], d.get('ms_per_step_repeats'), c['launch'][:10], k)" 2>&1 | tail -1)"
  done
  if [ -n "${SERIAL:-}" ]; then
    line=$(tools/variant.sh -t 300 -s "$SOURCES" -x "$ex" -- python3 tools/fused_variants.py | tail -1) || exit $?
    echo "[$ex] serial: $(echo "$line" | cut -c1-330)"
  fi
done <<< "${VARIANTS:-}"
