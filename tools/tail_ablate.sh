#!/bin/bash
# Tuning aid: tail_chain_kernel without its weight stream (-DTC_NOWLOAD, wrong results): what the k-group prefetch leaves
# exposed
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for ex in "" "-DTC_NOWLOAD"; do
  line=$(LPF_CFG=${1:-collab} tools/variant.sh -t 300 -s tail_chain -x "$ex" -- python3 tools/fused_variants.py | tail -1) || exit $?
  echo "[$ex] $(echo "$line" | grep -o '"tail_chain": [0-9.]*')"
done
