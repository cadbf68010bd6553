#!/bin/sh
# The host statement of the strict FASTA / FASTQ record parser (c3poa_amd/csrc/c3_fastx.cpp + c3_fastx.h) compiled for the CPU
# with AddressSanitizer and UBSan as a stand-alone program (tools/post_text_fuzz_host.cpp): texts of both kinds with random cuts
# and byte edits, every result held against the program's own plain reimplementation of the rule, every buffer a heap block of
# its exact size.  Host code only: nothing is loaded into Python and nothing runs on a GPU.
#   tools/post_text_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/post_text_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_fastx.cpp" -o "$TMP/fuzz"
"$TMP/fuzz" "$N" "$SEED"
