#!/bin/bash
# Developer check for a CPU machine: the weight packer (weights_pack.hip, compiled as plain C++), the derived-weights tables and routine of
# weights_layout.h, and pack_check.cpp under the address and undefined-behaviour sanitizers, built into build/pack_check next to this script and run.  No GPU, no HIP runtime.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
CXX="${CXX:-/opt/rocm/lib/llvm/bin/clang++}"
mkdir -p "$HERE/build"
$CXX -x c++ -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=all \
  -Wall -o "$HERE/build/pack_check" "$HERE/pack_check.cpp" "$HERE/weights_pack.hip"
"$HERE/build/pack_check"
