#!/bin/sh
# Host sanitizer check of c3_emit_group_bam_host against the writer whose records it restates as BAM: compiles
# c3poa_amd/csrc/c3_bamout.cpp, c3_emit.cpp, c3_writer.cpp and tools/bam_out_fuzz_host.cpp for the CPU with AddressSanitizer and
# UndefinedBehaviorSanitizer, runs a few thousand random and hostile record tables through the call, decodes every record with
# the plain decoder of the .cpp and compares it with the writer's text (see the .cpp).  A stand-alone program: nothing is loaded
# into Python and nothing runs on a GPU (hipcc only because the library is built with it: these units need no HIP header).
#   tools/bam_out_fuzz_host.sh [groups]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
$HIPCC -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Wall \
  "$ROOT/c3poa_amd/csrc/c3_bamout.cpp" "$ROOT/c3poa_amd/csrc/c3_emit.cpp" "$ROOT/c3poa_amd/csrc/c3_writer.cpp" "$ROOT/tools/bam_out_fuzz_host.cpp" -lz -o "$OUT/bam_out_fuzz_host"
# (the writer keeps its pooled arenas until the process ends, on purpose: no leak report)
ASAN_OPTIONS=detect_leaks=0 "$OUT/bam_out_fuzz_host" "${1:-4000}" "$OUT"
