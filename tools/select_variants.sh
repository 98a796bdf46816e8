#!/bin/bash
# Tuning aid: select3 build variants (one flag string per line of $VARIANTS, "" = the default build) x configs ->
# launch times + result digest
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
CONFIGS=${CONFIGS:-"collab ppa"}
while IFS= read -r ex; do
  for c in $CONFIGS; do
    line=$(LPF_CFG=$c tools/variant.sh -t 600 -s select3 -x "$ex" -- python3 tools/select_bench.py | tail -1) || exit $?
    echo "[$ex] $line"
  done
done <<< "${VARIANTS:-$'\n-DS3_PER_CU=3\n-DS3_PER_CU=4 -DS3_MIN_WAVES=4'}"
