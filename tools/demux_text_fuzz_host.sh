#!/bin/sh
# The host statement of the demultiplexer's text path (c3poa_amd/csrc/c3_dsplit.cpp + c3_dsplit.h, with the parsers c3_fasta.cpp and
# c3_fastx.cpp and the host compressor c3_bgzf.cpp under it) compiled for the CPU with AddressSanitizer and UBSan as a stand-alone
# program (tools/demux_text_fuzz_host.cpp), run on FASTA and FASTQ texts with random cuts and byte edits under every flag
# combination.  Every result is held against the tests' own Python models of the two rules (tests/demux_emit_cases.py: ref_parse;
# tests/demux_text_cases.py: ref_strict_fastq) and of the streams; every output buffer is a heap block of its exact size.
# Host code only: nothing is loaded into Python and malformed text is thrown at the rule here, never at a GPU.
#   tools/demux_text_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
C="$ROOT/c3poa_amd/csrc"
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/demux_text_fuzz_host.cpp" "$C/c3_dsplit.cpp" "$C/c3_fasta.cpp" "$C/c3_fastx.cpp" "$C/c3_bgzf.cpp" -x none -lz -o "$TMP/fuzz"
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP/cases.bin" "$N" "$SEED" <<'PY'
import struct, sys
import numpy as np
import demux_emit_cases as D
import demux_text_cases as T
path, n_cases, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(seed)
A = [b"", b"x", b"Nextera_7"]                                   # the driver's index names
B = [b"T1", b"", b"a name of sixty-four bytes" + b"." * 38]
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
long_recs = b"".join(b">read %d\n" % k + bytes(rng.choice(acgt, 280 + 9 * k)) + b"\n" for k in range(8))
wrapped = b"".join(b">w%d\r\n" % k + b"".join(bytes(rng.choice(acgt, 60)) + b"\r\n" for _ in range(4 + k)) for k in range(4))
fq_long = b"".join(b"@q%d c\n" % k + bytes(rng.choice(acgt, 290 + 7 * k)) + b"\n+\n" + T.qual_of(k, 290 + 7 * k) + b"\n" for k in range(8))
fq_crlf = fq_long.replace(b"\n", b"\r\n")
bases = {2: [t for _n, t in D.corpus() if t] + [long_recs, wrapped, long_recs + wrapped], 4: [fq_long, fq_crlf, T.to_fastq(long_recs)]}
edits = [b"\n", b"\r", b"\r\n", b">", b"@", b"+", b" ", b"\t", b"\x0b", b"\x1f", b"\x80", b"\xc3", b"A", b"|", b"\n\n", b"\n>", b"\n@", b""]
with open(path, "wb") as fh:
    for _ in range(n_cases):
        kind = 2 if rng.integers(2) else 4
        t = bytearray(bases[kind][int(rng.integers(len(bases[kind])))])
        for _k in range(int(rng.integers(0, 3))):
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
        flags = int(rng.integers(16)) & ~T.IN_BGZF
        if kind == 2:
            flags &= ~T.KEEP_QUALS
            recs, consumed, departed = D.ref_parse(t, bool(at_eof))
            recs = [(n, s, b"") for n, s in recs]
        else:
            recs, consumed, departed = T.ref_strict_fastq(t, bool(at_eof))
        S = 16 if flags & T.SPLIT else 1
        streams = [[] for _s in range(S)]
        n_kept = 0
        for nm, s, q in recs:
            if len(s) <= 300:
                continue
            n_kept += 1
            wa, wb = s[0] % 4 - 1, s[1] % 4 - 1
            head = nm + b"|" + A[wa] * (wa >= 0) + b"_" + B[wb] * (wb >= 0) + b"\n" + s + b"\n"
            rec = b"@" + head + b"+\n" + q + b"\n" if flags & T.KEEP_QUALS else b">" + head
            streams[((3 if wa < 0 else wa) * 4 + (3 if wb < 0 else wb)) if flags & T.SPLIT else 0].append(rec)
        streams = [b"".join(x) for x in streams]
        hs = np.array([D.fnv1a(r[0]) for r in recs], dtype="<u8")
        fh.write(struct.pack("<4q", len(t), at_eof, kind, flags) + t)
        fh.write(struct.pack("<5q", len(recs), consumed, departed, n_kept, S) + hs.tobytes())
        fh.write(np.array([len(x) for x in streams], dtype="<i8").tobytes() + b"".join(streams))
PY
"$TMP/fuzz" "$TMP/cases.bin"
