#!/bin/sh
# Digest of the groups and buffer sizes the streaming reader hands out (see the .cpp): compiles c3poa_amd/csrc/c3_reader.cpp,
# c3_reader_bgzf.cpp, c3_bam.cpp and tools/reader_digest_host.cpp for the CPU with AddressSanitizer and
# UndefinedBehaviorSanitizer, writes the inputs with tools/reader_digest_inputs.py and prints the digest of them all.  A
# stand-alone program: nothing is loaded into Python and nothing runs on a GPU (c3_hostbuf.h includes the HIP headers for its
# page-locked buffers, hence hipcc).  The committed digest is profiles/reader_digest.txt; a change of the reader that is meant
# to leave its groups and sizes alone prints the same bytes.
#   tools/reader_digest_host.sh > digest.txt          (folded: one line per input and group setting)
#   tools/reader_digest_host.sh -v > calls.txt       (one line per call, to find where two builds part)
#   READER_SOURCES="path/to/other/reader.cpp ..." tools/reader_digest_host.sh     (another build of the reader, same driver)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CSRC="$ROOT/c3poa_amd/csrc"
SOURCES=${READER_SOURCES:-"$CSRC/c3_reader.cpp $CSRC/c3_reader_bgzf.cpp $CSRC/c3_bam.cpp"}
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
# shellcheck disable=SC2086
$HIPCC -std=c++17 -O1 -g -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Wall \
  $SOURCES "$ROOT/tools/reader_digest_host.cpp" -lz -o "$OUT/reader_digest_host"
python3 "$ROOT/tools/reader_digest_inputs.py" "$OUT/in" > "$OUT/args"
# (file names, not their directory, go into the digest)
xargs "$OUT/reader_digest_host" $1 < "$OUT/args"
