"""What the tests of C3POa_demux.py --parse gpu share (tests/test_demux_text_host.py, tests/test_gpu_demux_text.py) and what
tools/demux_text_fuzz_host.sh holds the host statement against: texts of both kinds made from the golden demultiplexer cases,
the Python path (read_fasta / seqio.fastx_read -> demultiplex(host=True)) grouped by the '|A_B' suffix as the model of the
streams, and the feeding of pieces."""
import gzip
import os

import numpy as np

from c3poa_amd import _lib, demux, seqio
from demux_emit_cases import case_files, dedup, golden_cases, ref_parse

IN_BGZF, OUT_BGZF, KEEP_QUALS, SPLIT = _lib.DEMUX_IN_BGZF, _lib.DEMUX_OUT_BGZF, _lib.DEMUX_KEEP_QUALS, _lib.DEMUX_SPLIT


def qual_of(i, n):
    """varied qualities: every printable quality byte turns up, none is a line's first byte that would look like a header twice"""
    return bytes(33 + (i * 7 + j * 3) % 60 for j in range(n))


def to_fastq(text):
    """the records of a FASTA text (ASCII, not headless) as strict four-line FASTQ: blanks in a name become '_' (the FASTQ name
    ends at the first blank), repeated names and empty sequences are left out, qualities vary"""
    recs, _c, _d = ref_parse(text, True)
    seen, out = set(), []
    for name, seq in recs:
        name = name.replace(b" ", b"_").replace(b"\t", b"_")
        if name in seen or not seq or not name:
            continue
        seen.add(name)
        out.append(b"@" + name + b" comment %d\n" % len(out) + seq + b"\n+\n" + qual_of(len(out), len(seq)) + b"\n")
    return b"".join(out)


def ref_strict_fastq(text, at_eof):
    """the strict four-line rule of c3_fastq.h / c3_fastx.h (kind 4) in Python: (records [(name, sequence, quality)], consumed,
    departed) -- the longest prefix of whole strict records; an incomplete record is left alone unless the file ends"""
    recs, p, n, departed = [], 0, len(text), 0
    while p < n or (at_eof and p == n):
        lines, q, raw_end = [], p, p
        while len(lines) < 4:
            nl = text.find(b"\n", q) if q < n else -1
            if nl < 0 and not (at_eof and q < n):
                break
            raw_end = nl if nl >= 0 else n
            lines.append(text[q:raw_end - 1] if raw_end > q and text[raw_end - 1:raw_end] == b"\r" else text[q:raw_end])
            q = raw_end + 1 if nl >= 0 else n + 1
        if len(lines) < 4:
            if at_eof and lines:
                departed = 1
            break
        l0, l1, l2, l3 = lines
        strict = l0[:1] == b"@" and l1 and l1[:1] not in (b"@", b">", b"+") and l2[:1] == b"+" and len(l3) == len(l1)
        if not strict or any(c >= 0x80 for c in text[p:raw_end]):
            departed = 1
            break
        p = min(q, n)
        name = l0[1:]
        for k, c in enumerate(name):
            if c in b" \t":
                name = name[:k]
                break
        recs.append((name, l1, l3))
        if p == n and at_eof:
            break
    return recs, p, departed


def golden_texts(tmp):
    """[(tag, kind, text, nextera file, tso file)] for custom_indexes, empty_index and the de-duplicated paper case, as FASTA
    and converted to FASTQ"""
    gold = {c["name"]: c for c in golden_cases()}
    out = []
    for name in ("custom_indexes", "empty_index", "paper"):
        inp, nx, tso = case_files(gold[name], tmp)
        text = dedup(open(inp, "rb").read()) if name == "paper" else open(inp, "rb").read()
        out.append((name, 2, text, nx, tso))
        out.append((name + "_fq", 4, to_fastq(text), nx, tso))
    return out


def small_text(kind, tmp, n=3):
    """(text, nextera, tso): n records cut from the golden paper reads to 301, 300 (not kept), 320, ... bases and the first two
    indexes of each golden set, so that cutting the text at every byte stays cheap (a call searches two heads for four indexes);
    the FASTA text wrapped at 60 columns with CRLF"""
    gold = {c["name"]: c for c in golden_cases()}
    inp, nx_all, tso_all = case_files(gold["paper"], tmp)
    nx, tso = os.path.join(str(tmp), "small_nextera.fasta"), os.path.join(str(tmp), "small_tso.fasta")
    for src, dst in ((nx_all, nx), (tso_all, tso)):
        names, seqs = demux.load_indexes(src)
        with open(dst, "w") as f:
            f.write("".join(">%s\n%s\n" % (a, b) for a, b in list(zip(names, seqs))[:2]))
    recs = [r for r in ref_parse(dedup(open(inp, "rb").read()), True)[0] if len(r[1]) > 340][:n]
    lens = [301, 300, 320, 333, 302, 299][:n]
    out = []
    for i, ((name, seq), ln) in enumerate(zip(recs, lens)):
        seq = seq[:ln]
        if kind == 2:
            out.append(b">" + name + b"\r\n" + b"".join(seq[k:k + 60] + b"\r\n" for k in range(0, ln, 60)))
        else:
            out.append(b"@" + name.replace(b" ", b"_") + b"\n" + seq + b"\n+\n" + qual_of(i, ln) + b"\n")
    return b"".join(out), nx, tso


def stream_table(nx, tso):
    """{'<A>_<B>': stream index} and S for the index files: stream a * (n_b + 1) + b, the empty field last in each set"""
    a_names, b_names = demux.load_indexes(nx)[0] + [""], demux.load_indexes(tso)[0] + [""]
    return {a + "_" + b: ia * len(b_names) + ib for ia, a in enumerate(a_names) for ib, b in enumerate(b_names)}, len(a_names) * len(b_names)


def model_streams(text, kind, nx, tso, tmp, flags=0, tag="m"):
    """the plain streams of `text` by the Python path: read_fasta or fastx_read (dict semantics), demultiplex(host=True), the
    records formatted and grouped by their suffix; (streams, records in the file)"""
    p = os.path.join(str(tmp), tag + (".fa" if kind == 2 else ".fq"))
    with open(p, "wb") as f:
        f.write(text)
    quals = {}
    if kind == 2:
        reads = demux.read_fasta(p)
    else:
        reads = {}
        for name, seq, q in seqio.fastx_read(p):
            reads[name], quals[name] = seq, q
    indexed = demux.demultiplex(reads, nx, tso, host=True)
    kept = [n for n, s in reads.items() if len(s) > demux.HEAD]
    assert len(kept) == len(indexed)
    table, S = stream_table(nx, tso)
    streams = [[] for _ in range(S if flags & SPLIT else 1)]
    for name, (new, seq) in zip(kept, indexed.items()):
        rec = "@%s\n%s\n+\n%s\n" % (new, seq, quals[name]) if flags & KEEP_QUALS else ">%s\n%s\n" % (new, seq)
        streams[table[new[len(name) + 1:]] if flags & SPLIT else 0].append(rec.encode("latin-1"))
    return [b"".join(s) for s in streams], len(reads)


def compressed(streams):
    """every non-empty stream as the members c3_bgzf_compress_host makes of it"""
    return [_lib.bgzf_compress_host(s) if s else b"" for s in streams]


def feed_pieces(emit, text, fresh):
    """a statement fed `fresh` new bytes per call plus the unconsumed tail: (streams, hashes, calls); emit(text, at_eof) -> DemuxText"""
    streams, hashes, tail, pos, calls = None, [], b"", 0, 0
    while True:
        new = text[pos:pos + fresh]
        pos += len(new)
        at_eof = pos >= len(text)
        r = emit(tail + new, at_eof)
        calls += 1
        assert r.info["departed"] == 0 and r.guards_intact
        got = r.streams()
        streams = got if streams is None else [a + b for a, b in zip(streams, got)]
        hashes.append(r.hashes)
        tail = (tail + new)[r.info["consumed"]:]
        if at_eof:
            assert tail == b""
            return streams, np.concatenate(hashes), calls


def records_of(stream, keep_quals):
    """the records of a plain output stream (sequences and qualities are single lines)"""
    lines = stream.split(b"\n")
    assert lines[-1] == b""
    k = 4 if keep_quals else 2
    assert (len(lines) - 1) % k == 0
    return [b"\n".join(lines[i:i + k]) + b"\n" for i in range(0, len(lines) - 1, k)]


def gunzip_members(data):
    """the text of a chain of gzip members"""
    return gzip.decompress(data) if data else b""
