#!/bin/sh
# The host statement of k_fastq (c3poa_amd/csrc/c3_fastq.cpp + c3_fastq.h) compiled for the CPU with AddressSanitizer and
# UBSan, run on FASTQ text with random cuts and byte edits (newlines, '@', '+', '>', '\r', blanks put in or taken out), every
# result held against the tests' own Python parser of the strict rule (tests/test_fastq_host.py: ref_parse).
# Host code only: the rule is the one the kernels apply, so malformed text is thrown at it here, never at a GPU.
#   tools/fastq_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/fastq_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_fastq.cpp" -o "$TMP/fuzz"
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP/cases.bin" "$N" "$SEED" <<'PY'
import struct, sys
import numpy as np
import test_fastq_host as F
path, n_cases, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(seed)
bases = [t for _n, t, _e, _m in F.valid_corpus() if t] + [t for _n, t, _e, _s, _p in F.departure_corpus()]
edits = [b"\n", b"\r", b"\r\n", b"@", b"+", b">", b" ", b"\t", b"A", b"\n\n", b""]
with open(path, "wb") as fh:
    for _ in range(n_cases):
        t = bytearray(bases[int(rng.integers(len(bases)))])
        for _k in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(t) + 1))
            e = edits[int(rng.integers(len(edits)))]
            if rng.integers(2):
                t[at:at] = e                                   # put in
            else:
                t[at:at + 1] = e                               # replace (or, with the empty edit, take out)
        if rng.integers(3) == 0:
            t = t[:int(rng.integers(0, len(t) + 1))]           # cut
        t = bytes(t)
        at_eof, min_len = int(rng.integers(2)), int(rng.choice([0, 0, 3, 64, 300]))
        recs, n_short, consumed, departed = F.ref_parse(t, bool(at_eof), min_len)
        names, seqs, quals = (b"".join(r[k] for r in recs) for k in range(3))
        no = np.cumsum([0] + [len(r[0]) for r in recs]).astype("<i8")
        so = np.cumsum([0] + [len(r[1]) for r in recs]).astype("<i8")
        fh.write(struct.pack("<3q", len(t), at_eof, min_len) + t)
        fh.write(struct.pack("<7q", len(recs) + n_short, len(recs), n_short, consumed, len(names), len(seqs), departed))
        fh.write(names + seqs + quals + no.tobytes() + so.tobytes())
PY
"$TMP/fuzz" "$TMP/cases.bin"
