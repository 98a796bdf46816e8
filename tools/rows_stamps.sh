#!/bin/bash
# phase marks of pair_rows_kernel: tools/rows_stamps.sh "<extra -D flags>" [config]
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
LPF_CFG=${2:-collab} tools/variant.sh -t 600 -s pair_rows -x "-DPR_STAMPS $1" -- python3 tools/rows_stamps.py 2>&1 | grep -v amdgpu.ids
