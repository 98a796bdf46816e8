#!/bin/bash
# pair_rows timing builds: -DPR_ABL_NOFLIP = neither detection nor correction of flipped hidden units (wrong results),
# -DPR_ABL_ALLDETECT = every entry looks at its units, as before the no-flip box (right results)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for ex in "" "-DPR_ABL_ALLDETECT" "-DPR_ABL_NOFLIP" "-DPR_ABL_NOZ" "-DPR_ABL_NOFLIP -DPR_ABL_NOZ"; do
  line=$(tools/variant.sh -t 300 -s pair_rows -x "$ex" -- python3 bench.py --full --gpus 1 --steps 40 --warmup 5 --rows on --launch plan --weights random --no-bf16 --no-cpu-baseline | tail -1) || exit $?
  [ -n "$line" ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
  echo "[$ex] $(echo "$line" | python3 tools/all_configs_fmt.py | head -2 | cut -c1-110 | tr '\n' ' ')"
done
