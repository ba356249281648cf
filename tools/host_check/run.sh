#!/bin/bash
# Host-side sanitizer run of the library's argument and descriptor logic (no GPU needed, none
# used): the library's host code and each stand-alone program here under AddressSanitizer and
# UBSan. field_variants.cpp walks the fused field's descriptors, sparse_volume.cpp the
# refusals of the sparse volume's entries, of the two marchers and of the light-volume entries.
#   bash tools/host_check/run.sh [build dir]
set -euo pipefail
HERE=$(cd "$(dirname "$0")" && pwd)
CSRC=$HERE/../../atmospheric-neural-rendering_amd/csrc
OUT=${1:-$HERE/build}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$OUT/lib"
for f in encodings mlp mlp_fused field_fused volume_render sparse_volume; do
  extra=""
  [ "$f" = field_fused ] && extra="-fno-honor-nans -mno-amdgpu-ieee -mllvm -amdgpu-mfma-vgpr-form=1"
  $HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -fPIC $SAN $extra -c "$CSRC/$f.hip" -o "$OUT/lib/$f.o" &
done
wait
for prog in field_variants sparse_volume; do
  $HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 $SAN -x hip -c "$HERE/$prog.cpp" -o "$OUT/$prog.o"
  $HIPCC --offload-arch=gfx950 -fsanitize=address,undefined "$OUT"/lib/*.o "$OUT/$prog.o" -o "$OUT/$prog"
  "$OUT/$prog"
done
