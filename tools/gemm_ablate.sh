#!/bin/bash
# Tuning aid: gemm_f32.hip with one part compiled out (wrong results, timing only).
#   tools/gemm_ablate.sh      the encoder's unfused GEMM (GR_NOLOAD / GR_NOSTORE / GR_NOMFMA) under tools/enc_time.py
#   tools/gemm_ablate.sh tn   lpf_gemm_tn_f32's partial kernel alone (rocprofv3 kernel trace of tools/gemm_tn_bench.py):
#                             the shipped build, the matrix work alone (-DLPF_TN_NOLOAD) and the loads alone
#                             (-DLPF_TN_NOMFMA), each with its reduce kernel
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
if [ "${1:-}" = tn ]; then
  for ex in "" "-DLPF_TN_NOLOAD" "-DLPF_TN_NOMFMA"; do
    rm -rf /tmp/tnp
    tools/variant.sh -t 300 -s gemm_f32 -x "$ex" -- rocprofv3 --kernel-trace --output-format csv -d /tmp/tnp -- python3 tools/gemm_tn_bench.py > /dev/null || exit $?
    [ -d /tmp/tnp ] || continue   # (VARIANT_BUILD_ONLY=1: nothing ran)
    echo "[$ex]"; python3 tools/kernel_median.py /tmp/tnp gemm_tn
  done
  exit 0
fi
for ex in "" "-DGR_NOLOAD" "-DGR_NOSTORE" "-DGR_NOMFMA" "-DGR_NOLOAD -DGR_NOSTORE"; do
  line=$(LPF_FUSED=0 tools/variant.sh -t 300 -s gemm_f32 -x "$ex" -- python3 tools/enc_time.py | tail -1) || exit $?
  echo "[$ex] $line"
done
