#!/bin/bash
# Tuning aid: ablations of gcn_fused_kernel (GF_NOMFMA: no product, GF_NOGATHER: no neighbour loads)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for ex in "" "-DGF_NOMFMA" "-DGF_NOGATHER" "$@"; do
  line=$(tools/variant.sh -t 300 -s gcn_fused -x "$ex" -- python3 tools/enc_time.py | tail -1) || exit $?
  echo "[$ex] $line"
done
