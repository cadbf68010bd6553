"""Shared cases of test_bam_out_host.py and test_gpu_bam_out.py (--bam: the records of --emit gpu as unaligned BAM).  The
yardstick is the text the EXISTING writer makes of a group (emit_cases.written_files): a small pure-Python decoder turns BAM
record bytes into fields, a small text parser turns the writer's FASTA / FASTQ into the fields those records must hold.
Groups for the seams the text path does not have (packed bases, the quality clamp, name limits) are added to those of
emit_cases.  Nothing here calls the code under test."""
import gzip
import struct

import numpy as np

import emit_cases as EC
from c3poa_amd import _lib

CODES = "=ACMGRSVTWYHKDBN"
TX_LONG = 32768                                                   # k_text.h: reads above it are shared by the waves of a workgroup
SEAM_LENS = list(range(10)) + [127, 128, 129, 255, 256, 257]
QUAL_BYTES = [0, 32, 33, 126, 127, 255]
MAX_NAME = 219


def base_letter(c):
    """the letter a BAM reader shows for text byte c: itself (upper case) when it is one of CODES, else N"""
    if 97 <= c <= 122:
        c -= 32
    return chr(c) if c < 128 and chr(c) in CODES else "N"


def mapped(seq):
    return "".join(base_letter(c) for c in seq)


def clamped(qual):
    return bytes(min(max(c - 33, 0), 93) for c in qual)


def decode_records(data):
    """every record of an uncompressed stream: the block sizes must chain to its end exactly, the fixed fields hold their
    stated values.  -> [dict(name, seq, qual, tags, at, l_seq)] with seq as letters, at = offset of the record"""
    out, p = [], 0
    while p < len(data):
        assert p + 36 <= len(data), "a record's fixed part crosses the end of the stream"
        bs, ref, pos, lrn, mapq, bn, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", data, p)
        assert (ref, pos, mapq, bn, ncig, flag, nref, npos, tlen) == (-1, -1, 0, 4680, 0, 4, -1, -1, 0), (p, ref, pos, mapq, bn, ncig, flag, nref, npos, tlen)
        end = p + 4 + bs
        assert lrn >= 1 and lseq >= 0 and end <= len(data), (p, bs, lrn, lseq)
        q = p + 36
        name = data[q:q + lrn]
        assert name[-1:] == b"\0" and b"\0" not in name[:-1], name
        q += lrn
        nb = (lseq + 1) // 2
        pk = data[q:q + nb]
        seq = "".join(CODES[b >> 4] + CODES[b & 15] for b in pk)[:lseq]
        if lseq & 1:
            assert pk[-1] & 15 == 0, "the unused low nibble is not 0"
        q += nb
        qual = data[q:q + lseq]
        q += lseq
        assert q <= end, (p, "the fields are longer than block_size says")
        out.append(dict(name=name[:-1], seq=seq, qual=qual, tags=data[q:end], at=p, l_seq=lseq))
        p = end
    assert p == len(data)
    return out


def decode_tags(tags):
    """np:i rl:i aq:f in this order -> (np, rl, aq as numpy.float32)"""
    assert len(tags) == 21 and tags[0:3] == b"npi" and tags[7:10] == b"rli" and tags[14:17] == b"aqf", tags
    return struct.unpack_from("<i", tags, 3)[0], struct.unpack_from("<i", tags, 10)[0], np.frombuffer(tags[17:21], dtype="<f4")[0]


def inflate_members(data):
    """the bytes of concatenated BGZF (gzip) members"""
    return gzip.decompress(data) if data else b""


def parse_bam_file(data):
    """a whole .bam file -> (header text, records); the last 28 bytes must be the BGZF EOF member"""
    assert data[-28:] == _lib.BGZF_EOF, "no EOF member at the end"
    raw = inflate_members(data)
    assert raw[:4] == b"BAM\1"
    lt = struct.unpack_from("<i", raw, 4)[0]
    assert struct.unpack_from("<i", raw, 8 + lt)[0] == 0
    return raw[8:8 + lt], decode_records(raw[12 + lt:])


def reader_records(path):
    """every record the project's reader delivers from a file (FASTQ or BAM): [(name, bases, qualities)]"""
    import ctypes as C
    rd = _lib.Reader(path, n_sets=1)
    out = []
    try:
        while True:
            hb = rd.next(1000, 0, 0)
            if hb.n == 0:
                return out
            no, o = [int(x) for x in hb.name_off], [int(x) for x in hb.off]
            names, sq, ql = C.string_at(hb.c.names, no[-1]), C.string_at(hb.c.seqs, o[-1]), C.string_at(hb.c.quals, o[-1])
            out += [(names[no[i]:no[i + 1]], sq[o[i]:o[i + 1]], ql[o[i]:o[i + 1]]) for i in range(hb.n)]
    finally:
        rd.close()


# ---- the writer's text -> the fields the records must hold
def parse_fasta(text):
    """c3_write_group's consensus file: >name_avgQ_L_ns_clen \\n cons \\n; the length is taken from the header, so that a
    consensus may hold any byte.  -> [(header text, cons bytes)]"""
    out, p = [], 0
    while p < len(text):
        assert text[p:p + 1] == b">"
        e = text.index(b"\n", p)
        hd = text[p + 1:e]
        n = int(hd.rsplit(b"_", 1)[1])
        assert text[e + 1 + n:e + 2 + n] == b"\n"
        out.append((hd, text[e + 1:e + 1 + n]))
        p = e + 2 + n
    return out


def parse_cons_fastq(text):
    """c3_write_consensus_fastq's file, lengths from the header as parse_fasta -> [(header text, cons, qv)]"""
    out, p = [], 0
    while p < len(text):
        assert text[p:p + 1] == b"@"
        e = text.index(b"\n", p)
        hd = text[p + 1:e]
        n = int(hd.rsplit(b"_", 1)[1])
        s = e + 1
        assert text[s + n:s + n + 3] == b"\n+\n" and text[s + 2 * n + 3:s + 2 * n + 4] == b"\n"
        out.append((hd, text[s:s + n], text[s + n + 3:s + 2 * n + 3]))
        p = s + 2 * n + 4
    return out


def parse_sub_fastq(text):
    """c3_write_group's subread file: @name_idx \\n seq \\n+\\n qual \\n with |seq| = |qual| = the smallest n that fits and is
    followed by the end or by '@' (bases and qualities may hold a newline; no case here holds the three bytes \\n+\\n in
    a sequence) -> [(header text, seq, qual)]"""
    out, p = [], 0
    while p < len(text):
        assert text[p:p + 1] == b"@"
        e = text.index(b"\n", p)
        s, n = e + 1, 0
        while True:
            n = text.index(b"\n+\n", s + n) - s
            z = s + 2 * n + 3
            if text[z:z + 1] == b"\n" and (z + 1 == len(text) or text[z + 1:z + 2] == b"@"):
                break
            n += 1
        out.append((text[p + 1:e], text[s:s + n], text[s + n + 3:z]))
        p = z + 1
    return out


def read_key(header):
    """the read's name in a consensus header: without _avgQ_L_ns_clen"""
    return header.rsplit(b"_", 4)[0]


def quality_sums(group):
    """{read name: (tot, L)} of a Group, tot = sum of the read's quality bytes - 33 L (what the header's avgQ is made from)"""
    return {nm: (sum(q) - 33 * len(q), len(q)) for nm, q in zip(group.names, group.quals)}


def expected_records(written, with_qv, n_splints=EC.N_SPLINTS):
    """the writer's files (emit_cases.written_files) -> per splint (consensus records, subread records) as (name, letters, qual
    bytes or None); None = no QVs: l_seq bytes of 0xFF"""
    K = 3 if with_qv else 2
    out = []
    for s in range(n_splints):
        fa = parse_fasta(written[s * K])
        cons = [(hd, mapped(c), None) for hd, c in fa]
        if with_qv:
            fq = parse_cons_fastq(written[s * K + 2])
            assert [(hd, c) for hd, c, _q in fq] == fa
            cons = [(hd, mapped(c), clamped(q)) for hd, c, q in fq]
        subs = [(hd, mapped(sq), clamped(q)) for hd, sq, q in parse_sub_fastq(written[s * K + 1])]
        out.append((cons, subs))
    return out


# ---- groups for the seams of the BAM form
def seam_group():
    """subread pieces of SEAM_LENS bases, each at the four source alignments, four times in a row under names of odd and of
    even length (a record length that is odd walks the four destination alignments); consensuses of the same lengths at the
    four source alignments, brought there by short reads in between"""
    g = EC.Group(seed=21)
    for sa in range(4):
        for name in (b"ab", b"abc"):                              # 3 and 4 bytes with the digit
            base = sum(len(s) for s in g.seqs)                    # where this read's bases begin in the group
            subs, at = [(k, k + 11) for k in range(9)], 24        # nine fillers: the records below all have two-digit indexes
            for ln in SEAM_LENS:
                for _rep in range(4):
                    at += (sa - base - at) % 4
                    subs.append((at, at + ln))
                    at += ln + 1
            g.add("seam", at + 9, 0, subs=subs, clen=0, name=name + b"%d" % sa)
    total = 0
    for ln in SEAM_LENS:
        for sa in range(4):
            pad = (sa - total) % 4
            if pad:
                g.add("pad", 30, 0, subs=[(0, 10), (10, 30)], clen=pad)
                total += pad
            g.add("cons%d_%d" % (ln, sa), 40, 0, subs=[(0, 20), (20, 40)], clen=ln, name=b"c" * (1 + (ln + sa) % 5) + b"%d.%d" % (ln, sa))
            total += ln
    return g


def long_group():
    """reads around TX_LONG with pieces and consensuses of odd length: above it the four waves of a workgroup share every
    segment, in rows of the packed bytes"""
    g = EC.Group(seed=22)
    g.add("below", TX_LONG - 1, 0, subs=[(0, TX_LONG - 1)], clen=12001)
    g.add("at", TX_LONG, 1, subs=[(1, TX_LONG)], front=1, clen=12003)
    g.add("above", TX_LONG + 1, 0, subs=[(0, TX_LONG + 1), (3, 30000), (2, 1027)], front=513, tail=TX_LONG - 1026, clen=TX_LONG + 1)
    g.add("above2", TX_LONG + 700, 1, subs=[(5, TX_LONG + 698), (7, 520)], tail=TX_LONG + 699, clen=2049)
    g.add("short_between", 90, 0, subs=[(1, 40), (40, 81)], clen=33)
    return g


def bytes_group():
    """every byte value as a base (in a subread and in a consensus), at the four source alignments; the stated quality bytes
    as subread qualities and as QVs"""
    g = EC.Group(seed=23)
    allb = bytes(range(256))
    qq = bytes(QUAL_BYTES) * 44
    for sa in range(4):
        g.add("bytes%d" % sa, 260 + sa, sa & 1, subs=[(sa, sa + 256), (sa + 1, sa + 250)], front=sa, clen=256 + sa)
        g.seqs[-1] = b"a" * sa + allb + b"ACGT"
        g.quals[-1] = qq[:260 + sa]
        g.cons[-1] = allb[sa:] + allb[:sa] + b"n" * sa
        g.qv[-1] = (qq[sa:] + qq)[:256 + sa]
    return g


GROUPS = dict(EC.GROUPS, seams=seam_group, long=long_group, bytes=bytes_group)


def acgtn_group(n=40):
    """reads the project's BAM reader accepts back: ACGTN bases, qualities >= 33, no empty piece"""
    g = EC.Group(seed=24)
    for i in range(n):
        L = 120 + 7 * i
        g.add("rt", L, i & 1, subs=[(3, 50 + i), (50 + i, L - 2)], front=3, tail=L - 2, clen=40 + i)
        g.seqs[-1] = np.frombuffer(b"ACGTN", dtype=np.uint8)[g.rng.integers(0, 5, L)].tobytes()
    return g


def named_group(name):
    g = EC.Group(seed=25)
    g.add("before", 80, 0, subs=[(0, 40), (40, 80)], clen=20)
    g.add("named", 80, 1, subs=[(0, 40), (40, 80)], clen=20, name=name)
    return g
