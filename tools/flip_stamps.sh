#!/bin/bash
# per-wavefront finish times of pair_flip_kernel: tools/flip_stamps.sh [config] "<extra -D flags>"
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
LPF_CFG=${1:-collab} tools/variant.sh -t 300 -s pair_flip -x "-DFL_STAMPS $2" -- python3 tools/flip_stamps.py | tail -2
