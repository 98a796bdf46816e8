#!/bin/bash
# phase marks of tail_chain_kernel: tools/tail_stamps.sh "<extra -D flags>" [config]
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
LPF_CFG=${2:-collab} tools/variant.sh -t 600 -s tail_chain -x "-DTC_STAMPS $1" -- python3 tools/tail_stamps.py 2>&1 | grep -v amdgpu.ids
