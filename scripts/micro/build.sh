#!/bin/bash
# usage: build.sh <out> [extra hipcc flags]
out=$1; shift
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 -I "$ROOT/industrial_nnmpc_2021_amd/csrc" \
  "$@" "$ROOT/scripts/micro/lambda_micro.hip" -o $out
