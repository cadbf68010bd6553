#!/bin/sh
# The host statements of k_fasta (c3poa_amd/csrc/c3_fasta.cpp + c3_fasta.h) compiled for the CPU with AddressSanitizer and
# UBSan, run on FASTA text with random cuts and byte edits ('\n', '\r', '>', blanks, the other strip-set bytes, 0x80 put in or
# taken out), every result held against the tests' own Python parser of the rule (tests/demux_emit_cases.py: ref_parse).
# Host code only: the rule is the one the kernels apply, so malformed text is thrown at it here, never at a GPU.
#   tools/demux_emit_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/demux_emit_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_fasta.cpp" -o "$TMP/fuzz"
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP/cases.bin" "$N" "$SEED" <<'PY'
import struct, sys
import numpy as np
import demux_emit_cases as D
path, n_cases, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(seed)
A = [b"", b"x", b"Nextera_7"]                                   # the driver's index names
B = [b"T1", b"", b"a name of sixty-four bytes" + b"." * 38]
long_recs = b"".join(b">read %d\n" % k + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 280 + 9 * k)) + b"\n" for k in range(8))
wrapped = b"".join(b">w%d\r\n" % k + b"".join(bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 60)) + b"\r\n" for _ in range(4 + k)) for k in range(4))
bases = [t for _n, t in D.corpus() if t] + [long_recs, wrapped]
edits = [b"\n", b"\r", b"\r\n", b">", b" ", b"\t", b"\x0b", b"\x0c", b"\x1c", b"\x1f", b"\x80", b"\xc3", b"A", b"|", b"\n\n", b"\n>", b""]
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
        at_eof = int(rng.integers(2))
        recs, consumed, departed = D.ref_parse(t, bool(at_eof))
        names, seqs = (b"".join(r[k] for r in recs) for k in range(2))
        no = np.cumsum([0] + [len(r[0]) for r in recs]).astype("<i8")
        so = np.cumsum([0] + [len(r[1]) for r in recs]).astype("<i8")
        hs = np.array([D.fnv1a(r[0]) for r in recs], dtype="<u8")
        kept = [r for r in recs if len(r[1]) > 300]
        out = b"".join(b">" + nm + b"|" + A[s[0] % 4 - 1] * (s[0] % 4 > 0) + b"_" + B[s[1] % 4 - 1] * (s[1] % 4 > 0) + b"\n" + s + b"\n" for nm, s in kept)
        fh.write(struct.pack("<2q", len(t), at_eof) + t)
        fh.write(struct.pack("<5q", len(recs), consumed, len(names), len(seqs), departed))
        fh.write(names + seqs + no.tobytes() + so.tobytes() + hs.tobytes())
        fh.write(struct.pack("<2q", len(kept), len(out)) + out)
PY
"$TMP/fuzz" "$TMP/cases.bin"
