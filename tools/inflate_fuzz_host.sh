#!/bin/sh
# The host statement of k_inflate (c3poa_amd/csrc/c3_inflate.cpp + c3_inflate.h) compiled for the CPU with AddressSanitizer
# and UBSan, run on damaged BGZF members (random byte flips, truncated payloads), every verdict held against zlib's.
# Host code only: the decoder is the one the kernel runs, so damage is thrown at it here, never at a GPU.
#   tools/inflate_fuzz_host.sh [N_FLIPS=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/inflate_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_inflate.cpp" -o "$TMP/fuzz" -lz
# the members: the valid corpus of tests/test_inflate_host.py that the damaged corpus is drawn from, and more
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP/corpus.gz" <<'PY'
import sys, zlib
import test_inflate_host as H
fq = H.fastq_text()
far = dict(H.far_match_members())
ms = [H.bgzf_members(fq)[0], H.bgzf_members(fq, strategy=zlib.Z_FIXED)[0], H.bgzf_members(fq, level=0)[0],
      H.split_members(H._lib.bgzf_compress_host(fq))[0], H.handmade_member(far["far D=32768 L=258"]),
      H.handmade_member(far["far D=1 L=65"]), H.bgzf_members(fq, level=9, full_flush=True)[1], H.bgzf_members(fq, block=301)[3],
      H.bgzf_members(b"A" * 65280)[0]]
ms += [H.handmade_member(p) for _n, p in H.dynamic_header_members()]
open(sys.argv[1], "wb").write(b"".join(ms))
PY
"$TMP/fuzz" "$TMP/corpus.gz" "$N" "$SEED"
