#!/bin/bash
# where a block's time goes in select4_kernel: tools/select4_stamps.sh "<extra -D flags>" [config] [threads]
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
LPF_CFG=${2:-collab} LPF_SEL4_THREADS=${3:-0} tools/variant.sh -t 600 -s select4 -x "-DS4_STAMPS $1" -- python3 tools/select4_stamps.py 2>&1 | grep -v amdgpu.ids
