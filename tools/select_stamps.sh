#!/bin/bash
# where an item's time goes in select3_run_kernel: tools/select_stamps.sh "<extra -D flags>" [config]
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
LPF_CFG=${2:-collab} tools/variant.sh -t 600 -s select3 -x "-DS3_STAMPS $1" -- python3 tools/select_stamps.py 2>&1 | grep -v amdgpu.ids
