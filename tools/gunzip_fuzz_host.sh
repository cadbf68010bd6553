#!/bin/sh
# The host statement of the k_gunzip kernels (c3poa_amd/csrc/c3_gunzip.cpp: the procedure of c3_gunzip_run.h over the decoder
# of c3_gunzip.h) compiled for the CPU with AddressSanitizer and UBSan as a stand-alone program, run on cut and edited gzip
# files (byte flips, cuts at the end and out of the middle) at random piece sizes, verdict and bytes held against zlib linked
# into the same program.  Host code only: procedure and decoder are the ones the kernels run, so damage is thrown at them
# here, never at a GPU.
#   tools/gunzip_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/gunzip_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_gunzip.cpp" -o "$TMP/fuzz" -lz
# the files: small ones of every kind of tests/test_gunzip_host.py that the cut and edited ones are drawn from
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP" <<'PY'
import sys, zlib
import test_gunzip_host as H
fq = H.fastq_text()[:40000]
files = [H.gz(fq), H.gz(fq, 1, 1), H.gz(fq[:20000], 6, 8, zlib.Z_FIXED), H.gz(fq[:20000], 0), H.gz(fq, 6, 8, sync_every=1000),
         H.with_header(H.gz(fq[:20000]), extra=b"XY\x03\x00abc", name=b"n", comment=b"c", hcrc=True),
         H.gz(fq[:15000]) + H.gz(b"") + H.gz(fq[15000:30000], 9), H.gz(H.gz(fq), 0), H.copied_line_stream(),
         H.far_match_streams()[-1][1]]
for k, f in enumerate(files):
    open("%s/f%02d.gz" % (sys.argv[1], k), "wb").write(f)
PY
"$TMP/fuzz" "$N" "$SEED" "$TMP"/f*.gz
