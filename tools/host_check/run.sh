#!/bin/bash
# Host-side sanitizer run of the fused field's descriptor logic (no GPU needed, none used):
# the library's host code and field_variants.cpp under AddressSanitizer and UBSan, as one
# stand-alone program.   bash tools/host_check/run.sh [build dir]
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
CSRC=$HERE/../../atmospheric-neural-rendering_amd/csrc
OUT=${1:-$HERE/build}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$OUT"
for f in encodings mlp mlp_fused field_fused; do
  extra=""
  [ "$f" = field_fused ] && extra="-fno-honor-nans -mno-amdgpu-ieee -mllvm -amdgpu-mfma-vgpr-form=1"
  $HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC $SAN $extra -c "$CSRC/$f.hip" -o "$OUT/$f.o" &
done
wait
$HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 $SAN -x hip -c "$HERE/field_variants.cpp" -o "$OUT/field_variants.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT"/*.o -o "$OUT/field_variants"
"$OUT/field_variants"
