#!/bin/bash
# The one way to run something on a tuning build of the kernel library:
#   tools/variant.sh -t SECONDS [-s "sources"] [-x "flags"] [-n] -- command [args...]
# -x empty: `make` of the default build, the command runs on the installed library (LPF_HIP_LIB unset).
# -x "-D...": `make variant` compiles the sources of -s ("pair_rows tail_chain", or "all") with those flags into a library
#    of its own under lpformer_amd/csrc/build/variants/, and the command runs with LPF_HIP_LIB naming it.  The installed
#    library is never a variant, no source file is touched, and there is nothing to restore afterwards.
# One line on stderr names flags, sources and library before the command runs (under `timeout -k 10 SECONDS`).
# -n, or VARIANT_BUILD_ONLY=1 in the environment: build, print that line, exit 0 without running the command.
# Exit status: the command's (124 / 137 at the time limit); 64 for a usage error; 96 when the build failed -- the end of
# its log is printed and the command is NOT run.  Callers stop at the first non-zero status.  The log of the last build
# is lpformer_amd/csrc/build/variant_build.log, or the file VARIANT_LOG names.
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/.." || exit 64
usage() { echo "usage: tools/variant.sh -t SECONDS [-s \"sources\"] [-x \"flags\"] [-n] -- command [args...]" >&2; exit 64; }
limit="" src="" flags="" only=""
[ "${VARIANT_BUILD_ONLY:-}" = 1 ] && only=1
while getopts "t:s:x:n" o; do
  case $o in t) limit=$OPTARG ;; s) src=$OPTARG ;; x) flags=$OPTARG ;; n) only=1 ;; *) usage ;; esac
done
shift $((OPTIND - 1))
[ -n "$limit" ] || usage
[ -n "$only" ] || [ $# -gt 0 ] || usage
jobs=${MAX_JOBS:-8}; [ "$jobs" -le 16 ] || jobs=16
log=${VARIANT_LOG:-lpformer_amd/csrc/build/variant_build.log}; mkdir -p "$(dirname "$log")"
if [[ $flags =~ [^[:space:]] ]]; then
  [ -n "$src" ] || usage
  lib=$(make -C lpformer_amd/csrc -j"$jobs" variant VARIANT_SRC="$src" EXTRA="$flags" 2>&1 | tee "$log" | sed -n 's/^variant: //p') \
    && [ -f "$lib" ] && export LPF_HIP_LIB="$lib"
else
  src="" lib=$PWD/lpformer_amd/liblpformer_hip.so
  make -C lpformer_amd/csrc -j"$jobs" > "$log" 2>&1 && unset LPF_HIP_LIB
fi || { echo "[variant] build failed, flags='$flags' sources='$src'; the end of $log:" >&2; tail -20 "$log" >&2; exit 96; }
echo "[variant] flags='$flags' sources='$src' lib=$lib" >&2
[ -n "$only" ] && exit 0
timeout -k 10 "$limit" "$@"; rc=$?
[ $rc -eq 0 ] || echo "[variant] exit status $rc: $*" >&2
exit $rc
