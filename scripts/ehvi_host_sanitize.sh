#!/bin/bash
# ASan + UBSan over the HOST part of the EHVI (bo_hvi_boxes, bo_ehvi_tables, the argument checks of
# bo_expected_hypervolume_improvement): the library sources it needs compiled with the sanitizers
# on the host side only, linked with the stand-alone program scripts/ehvi_host_check.cpp, which is
# then run.  CPU only: every call returns before the first HIP call.
# Usage: scripts/ehvi_host_sanitize.sh [build_dir]
set -eu -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:-/tmp/bo_ehvi_sanitize}"
mkdir -p "$OUT"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined"
pids=()
for s in bo_ehvi bo_hvi; do
  $HIPCC --offload-arch=gfx950 -O1 -g -fno-omit-frame-pointer -std=c++17 -fPIC -I "$ROOT/include" $SAN \
    -c "$ROOT/bayesopt_smart_amd/csrc/$s.hip" -o "$OUT/$s.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
CLANGXX="${CLANGXX:-/opt/rocm/lib/llvm/bin/clang++}"      # the compiler behind hipcc: one sanitizer runtime
$CLANGXX -O1 -g -fno-omit-frame-pointer -std=c++17 -I "$ROOT/include" -fsanitize=address,undefined \
  -fno-sanitize-recover=undefined -c "$ROOT/scripts/ehvi_host_check.cpp" -o "$OUT/ehvi_host_check.o"
$HIPCC --offload-arch=gfx950 $SAN "$OUT"/ehvi_host_check.o "$OUT"/bo_ehvi.o "$OUT"/bo_hvi.o -o "$OUT/ehvi_host_check"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 "$OUT/ehvi_host_check"
