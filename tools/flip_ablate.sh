#!/bin/bash
# Tuning aid: ablations of pair_flip_kernel (FL_NOZ: no Z gather, FL_NOQ: no q loads, FL_NOCORR: no corrections)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for ex in "" "-DFL_NOCORR" "-DFL_NOZ" "-DFL_NOQ" "-DFL_NOZ -DFL_NOQ" "-DFL_NOZ -DFL_NOQ -DFL_NOCORR"; do
  line=$(LPF_CFG=${1:-collab} tools/variant.sh -t 300 -s pair_flip -x "$ex" -- python3 tools/fused_variants.py | tail -1) || exit $?
  echo "[$ex] $(echo "$line" | grep -o '"pair_attention_fused": [0-9.]*')"
done
