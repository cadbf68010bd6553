"""What the tests of C3POa_demux.py --emit gpu share (tests/test_demux_emit_host.py, tests/test_gpu_demux_emit.py) and what
tools/demux_emit_fuzz_host.sh holds the host statements against: a Python parser of the FASTA rule of c3poa_amd/csrc/c3_fasta.h,
the corpus of texts, and the Python host path as the reference of the emitted bytes."""
import bisect
import json
import os
import re

import numpy as np

from c3poa_amd import _lib, demux

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
STRIP = bytes([9, 10, 11, 12, 13, 28, 29, 30, 31, 32])          # what str.rstrip() takes off an ASCII line


def fnv1a(b):
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def ref_parse(text, at_eof):
    """the rule of c3_fasta.h in Python: (records [(name, sequence)], consumed, departed)"""
    lines, b = [], 0
    for m in re.finditer(b"[\r\n]", text):
        lines.append((b, text[b:m.start()]))
        b = m.end()
    lines.append((b, text[b:]))
    first_high = next((i for i, c in enumerate(text) if c >= 0x80), -1)
    recs, hb, first_headless = [], [], -1
    for b, raw in lines:
        s = raw.rstrip(STRIP)
        if not s:
            continue
        if s[:1] == b">":
            hb.append(b)
            recs.append([s[1:], b""])
        elif not recs:
            if first_headless < 0:
                first_headless = b
        else:
            recs[-1][1] += s
    n_head = len(recs)
    n_rec, departed = (n_head if at_eof else max(n_head - 1, 0)), 0
    if first_headless >= 0 and (first_high < 0 or first_headless <= first_high):
        departed, n_rec = 2, 0
    elif first_high >= 0:
        departed = 1
        n_rec = min(n_rec, max(bisect.bisect_right(hb, first_high) - 1, 0))
    if departed == 2:
        consumed = 0
    elif n_rec < n_head:
        consumed = hb[n_rec]
    else:
        consumed = len(text) if (at_eof and not departed) else 0
    return [tuple(r) for r in recs[:n_rec]], consumed, departed


SEMANTICS = b">r 1  \r\nACGT\r\n\r\nTT \n>r\t2\nGG\n  \n>r 1  \nCCC\rAA\n>x\n> \n A\n>empty\n"    # test_read_fasta_semantics


def corpus():
    """(name, text): every text starts at the start of a file; none is headless and none holds a byte >= 0x80"""
    wrapped = b"".join(b">w%d\n" % k + b"".join(b"ACGTTGCA"[j % 8:j % 8 + 1] * 7 + b"\n" for j in range(k)) for k in (1, 3, 9))
    out = [("semantics", SEMANTICS),
           ("wrapped", wrapped),
           ("crlf", b">a\r\nACGT\r\nTTGA\r\n>b\r\nGG\r\n"),
           ("lone_cr", b">a\rACGT\rTTGA\r>b\rGG\r"),
           ("strip_at_ends", b"".join(b">n%d%c\nAC%c\nGT\n" % (c, c, c) for c in STRIP if c not in (10, 13))),
           ("strip_inside", b"".join(b">n%cm\nA%cC\n" % (c, c) for c in STRIP if c not in (10, 13))),
           ("strip_runs", b">a \t\x0b\x0c\x1c\x1d\x1e\x1f \nAC \t \n \t\x1f\n\x0cGT\n"),
           ("empty_name", b">\nACGT\n> \nGG\n>\t\n"),
           ("empty_sequence", b">a\n>b\n\n\n>c\nAC\n>d\n"),
           ("no_final_newline", b">a\nACGT\n>b\nGG"),
           ("header_no_newline", b">a\nACGT\n>b"),
           ("leading_blank_lines", b"\n\r\n \t\n>r\nAC\nGT\n"),
           ("gt_inside", b">a>b\nAC>GT\n >c\n>d\n"),
           ("empty", b""),
           ("only_blank", b"\n \n\r\n")]
    return out


def golden_cases():
    return json.load(open(os.path.join(GOLD, "demux_cases.json")))["cases"]


def case_files(case, d):
    """input / Nextera / TSO paths of one golden case (texts written byte for byte, CR and CRLF kept)"""
    paths = []
    for key in ("input", "nextera", "tso"):
        v = case[key]
        if key != "input" and v.endswith(".fasta") and "\n" not in v:
            paths.append(os.path.join(GOLD, v))
            continue
        p = os.path.join(str(d), "%s_%s.fasta" % (case["name"], key))
        with open(p, "w", newline="") as f:
            f.write(v)
        paths.append(p)
    return paths


def sets_of(nextera_file, tso_file):
    a_names, a_seqs = demux.load_indexes(nextera_file)
    b_names, b_seqs = demux.load_indexes(tso_file)
    return _lib.DemuxSets(a_names, a_seqs, b_names, b_seqs)


def host_path_bytes(text, nextera_file, tso_file, d, tag="ref"):
    """Indexed_reads.fasta of the Python host path (read_fasta -> demultiplex(host=True) -> write_fasta_file) for `text`"""
    src = os.path.join(str(d), tag + "_in.fasta")
    with open(src, "wb") as f:
        f.write(text)
    out = os.path.join(str(d), tag + "_out")
    os.makedirs(out, exist_ok=True)
    demux.write_fasta_file(out, demux.demultiplex(demux.read_fasta(src), nextera_file, tso_file, host=True))
    with open(os.path.join(out, "Indexed_reads.fasta"), "rb") as f:
        return f.read()


def dedup(text):
    """`text` (ASCII, not headless) without the records whose header was seen before, as plain '>name\\nseq\\n' records"""
    recs, _c, _d = ref_parse(text, True)
    seen, out = set(), []
    for name, seq in recs:
        if name not in seen:
            seen.add(name)
            out.append(b">" + name + b"\n" + seq + b"\n")
    return b"".join(out)


def feed_chunks(emit, text, fresh):
    """c3_demux_emit fed as the CLI feeds it: `fresh` new bytes per call plus the unconsumed tail; (bytes, hashes, calls)"""
    out, hashes, tail, pos, calls = [], [], b"", 0, 0
    while True:
        new = text[pos:pos + fresh]
        pos += len(new)
        at_eof = pos >= len(text)
        r = emit(tail + new, at_eof)
        calls += 1
        assert r.info["departed"] == 0
        out.append(r.out)
        hashes.append(r.hashes)
        tail = (tail + new)[r.info["consumed"]:]
        if at_eof:
            assert tail == b""
            return b"".join(out), np.concatenate(hashes), calls
