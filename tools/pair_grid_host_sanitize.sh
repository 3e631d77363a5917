#!/bin/bash
# Builds tools/pair_grid_host_sanitize.hip with the host parts it needs under -fsanitize=address,undefined and runs it.  No GPU is used.
# The program is stand-alone: nothing loaded into python runs under a sanitizer.
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/build
mkdir -p "$out"
src=$root/se3et_amd/csrc
"${HIPCC:-/opt/rocm/bin/hipcc}" --offload-arch=gfx950 -O1 -g -std=c++17 -Wall -Wno-unused-function -ffp-contract=off \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  "$root/tools/pair_grid_host_sanitize.hip" "$src/pair_geometry.hip" "$src/knn_normals.hip" "$src/keypoint_nms.hip" "$src/capi_common.hip" \
  -o "$out/pair_grid_host_sanitize"
"$out/pair_grid_host_sanitize"
