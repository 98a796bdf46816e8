#!/bin/bash
# dense tail: 128 pairs per workgroup (one workgroup of 16 wavefronts per CU) against 64 (two of 8).
# (The kernel has since grown: with -DLPF_TC_GROUPS=8 its LDS no longer fits two workgroups per CU and the build stops at
# that static_assert -- the script then ends with the runner's build-failure status after the default build's two runs.)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
for ex in "" "-DLPF_TC_GROUPS=8"; do
  for i in 1 2; do
    line=$(tools/variant.sh -t 300 -s tail_chain -x "$ex" -- python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --rows on --launch plan --weights random --no-bf16 --no-cpu-baseline | tail -1) || exit $?
    [ -n "$line" ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
    echo "[$ex] $(echo "$line" | python3 tools/all_configs_fmt.py | head -2 | cut -c1-70 | tr '\n' ' ')"
  done
done
