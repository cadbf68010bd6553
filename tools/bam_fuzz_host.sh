#!/bin/sh
# The host statement of k_bam (c3poa_amd/csrc/c3_bam.cpp + c3_bam.h) compiled for the CPU with AddressSanitizer and UBSan, run
# on BAM bytes with random cuts and edits -- block_size, l_read_name, n_cigar_op, flag and l_seq above all, then any byte --
# every result held against the tests' own Python statement of the rule (tests/bam_cases.py: py_parse).
# Host code only: the rule is the one the kernels apply, so malformed data is thrown at it here, never at a GPU.
#   tools/bam_fuzz_host.sh [N_CASES=20000] [SEED=1]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-20000}
SEED=${2:-1}
CXX=${CXX:-c++}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
"$CXX" -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ \
  "$ROOT/tools/bam_fuzz_host.cpp" "$ROOT/c3poa_amd/csrc/c3_bam.cpp" -o "$TMP/fuzz"
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$TMP/cases.bin" "$N" "$SEED" <<'PY'
import struct, sys
import numpy as np
import bam_cases as B
path, n_cases, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(seed)
recs = B.valid_records()
values = {"<I": [0, 1, 33, 34, 35, 36, 40, 74, 255, 256, 65535, 65536, (1 << 28) - 1, 1 << 28, (1 << 28) + 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF],
          "<H": [0, 1, 2, 4, 0x10, 0x100, 0x800, 0x4D, 0x7FFF, 0xFFFF], "<B": [0, 1, 2, 7, 8, 254, 255]}
fields = [(0, "<I"), (12, "<B"), (16, "<H"), (18, "<H"), (20, "<I")]          # block_size, l_read_name, n_cigar_op, flag, l_seq
with open(path, "wb") as fh:
    for _ in range(n_cases):
        k = int(rng.integers(1, 7))
        pick = [recs[int(i)] for i in rng.integers(0, len(recs), k)]
        at_start = int(rng.integers(4) != 0)
        head = (B.header(b"@HD\n" * int(rng.integers(0, 3)), [(b"ref", 9)] * int(rng.integers(0, 3))) if at_start else b"")
        parts = [B.record(*a, **kw) for a, kw in pick]
        starts = np.cumsum([len(head)] + [len(p) for p in parts])[:-1]
        t = bytearray(head + b"".join(parts))
        for _e in range(int(rng.integers(0, 3))):
            kind = int(rng.integers(10))
            if kind < 7:                                               # a fixed field of one record
                at, fmt = fields[int(rng.integers(len(fields)))]
                v = values[fmt]
                struct.pack_into(fmt, t, int(starts[int(rng.integers(k))]) + at, v[int(rng.integers(len(v)))])
            elif kind < 9 and len(t):                                  # any byte
                t[int(rng.integers(len(t)))] = int(rng.choice([0, 1, 0x20, 0x09, 0xFF, int(rng.integers(256))]))
            elif len(head) >= 12:                                      # the header's lengths
                struct.pack_into("<i", t, int(rng.choice([4, len(head) - 4 if len(head) == 12 else 8])), int(rng.choice([-1, 0, 3, 1 << 20, 0x7FFFFFFF])))
        if rng.integers(3) == 0:
            t = t[:int(rng.integers(0, len(t) + 1))]                   # cut
        t = bytes(t)
        at_eof, min_len = int(rng.integers(2)), int(rng.choice([0, 0, 3, 64, 300]))
        w = B.py_parse(t, bool(at_start), bool(at_eof), min_len)
        rs = w["records"]
        names, seqs, quals = (b"".join(r[j] for r in rs) for j in range(3))
        no = np.cumsum([0] + [len(r[0]) for r in rs]).astype("<i8")
        so = np.cumsum([0] + [len(r[1]) for r in rs]).astype("<i8")
        fh.write(struct.pack("<4q", len(t), at_start, at_eof, min_len) + t)
        fh.write(struct.pack("<10q", w["n_records"], len(rs), w["n_short"], w["consumed"], len(names), len(seqs), w["header_bytes"],
                             w["bad_at"], w["departed"], w["reason"]))
        fh.write(names + seqs + quals + no.tobytes() + so.tobytes())
PY
"$TMP/fuzz" "$TMP/cases.bin"
