#!/bin/sh
# Host sanitizer check of c3_post_emit_host: compiles c3poa_amd/csrc/c3_post.cpp and tools/post_emit_fuzz_host.cpp with
# AddressSanitizer and UndefinedBehaviorSanitizer for the CPU and runs a few thousand random and hostile adapter tables through
# the host statement (see the .cpp).  A stand-alone program: nothing is loaded into Python and nothing runs on a GPU.
#   tools/post_emit_fuzz_host.sh [batches]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CXX=${CXX:-c++}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
$CXX -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall \
  "$ROOT/c3poa_amd/csrc/c3_post.cpp" "$ROOT/tools/post_emit_fuzz_host.cpp" -o "$OUT/post_emit_fuzz_host"
"$OUT/post_emit_fuzz_host" "${1:-3000}"
