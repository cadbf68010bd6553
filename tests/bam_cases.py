"""Unaligned BAM for the tests (include/c3poa.h "Unaligned BAM records on the GPU"): a writer built on struct
(the BGZF layer is test_inflate_host.bgzf_file), the tests' own statement of the rule (py_parse), the FASTQ text of the same
records (fastq_of: the yardstick is the FASTQ route, which was there before), and the named corpora that the host tests, the
host fuzz (tools/bam_fuzz_host.sh) and the GPU tests share.  No pysam, no samtools."""
import struct

import numpy as np

TILE = 65536                    # C3_BAM_TILE
MAX_RECORD = 1 << 28            # C3_BAM_MAX_RECORD
MAX_REFS = 1 << 20              # C3_BAM_MAX_REFS
CODES = "=ACMGRSVTWYHKDBN"
REASONS = ("OK", "BLOCK", "NAME", "FIELDS", "FLAG", "EMPTY", "NOQUAL", "TRUNCATED", "HEADER")
R = {n: i for i, n in enumerate(REASONS)}


# ---- writer ---------------------------------------------------------------------------------------------------------------
def header(text=b"", refs=()):
    """magic, l_text, text, n_ref, per reference l_name, name (NUL-terminated), l_ref"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def tag_bytes(n):
    """an optional field of exactly n bytes (n = 0, or n >= 8): XP:B:C with n - 8 bytes of 0xFF (no byte run of it looks like a
    record: block_size 0xFFFFFFFF is out of range)"""
    if n == 0:
        return b""
    assert n >= 8
    return b"XPBC" + struct.pack("<I", n - 8) + b"\xff" * (n - 8)


def record(name, seq, qual, flag=4, n_cigar=0, tags=b""):
    """one alignment record, block_size included.  name: bytes without the NUL; seq: str over CODES; qual: bytes of Phred values"""
    assert len(seq) == len(qual) and len(name) <= 254
    codes = [CODES.index(c) for c in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    cigar = b"".join(struct.pack("<I", (10 << 4) | 4) for _ in range(n_cigar))                  # 10S: any operations do
    body = (struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, n_cigar, flag, len(seq), -1, -1, 0)
            + name + b"\0" + cigar + packed + bytes(qual) + tags)
    return struct.pack("<I", len(body)) + body


def delivered(name, seq, qual):
    """what the rule delivers of record(name, seq, qual, ...): the name cut, the bases, the qualities as characters"""
    cut = len(name)
    for stop in (b"\0", b" ", b"\t"):
        k = name.find(stop)
        if k >= 0:
            cut = min(cut, k)
    return (name[:cut], seq.encode(), bytes(min(q, 93) + 33 for q in qual))


def fastq_of(recs):
    """the text @name\\nSEQ\\n+\\nQUAL\\n of (name, seq, qual) records as given to record()"""
    return b"".join(b"@" + n + b"\n" + s.encode() + b"\n+\n" + bytes(min(q, 93) + 33 for q in ql) + b"\n" for n, s, ql in recs)


# ---- the tests' own statement of the rule ---------------------------------------------------------------------------------
def py_header(data):
    """(status, bytes): 'ok', 'incomplete' or 'bad'"""
    n = len(data)
    if data[:4] != b"BAM\1"[:min(4, n)]:
        return "bad", 0
    if n < 8:
        return "incomplete", 0
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0:
        return "bad", 0
    p = 8 + l_text
    if p + 4 > n:
        return "incomplete", 0
    n_ref = struct.unpack_from("<i", data, p)[0]
    if n_ref < 0 or n_ref > MAX_REFS:
        return "bad", 0
    p += 4
    if n_ref > (n - p) // 8:                                   # 8 bytes a reference at least: it cannot end inside the data
        return "incomplete", 0
    for _ in range(n_ref):
        if p + 4 > n:
            return "incomplete", 0
        l_name = struct.unpack_from("<i", data, p)[0]
        if l_name < 0:
            return "bad", 0
        p += 8 + l_name
        if p > n:
            return "incomplete", 0
    return "ok", p


def py_record(data, p):
    """('ok', next, name, seq, qual) | ('incomplete',) | (reason name,) for the record at byte p"""
    n = len(data)
    if p + 4 > n:
        return ("incomplete",)
    bs = struct.unpack_from("<I", data, p)[0]
    if not 34 <= bs <= MAX_RECORD:
        return ("BLOCK",)
    if p + 4 + bs > n:
        return ("incomplete",)
    lrn = data[p + 12]
    nc, flag, ls = struct.unpack_from("<HHI", data, p + 16)
    if lrn == 0 or (32 + lrn <= bs and data[p + 36 + lrn - 1] != 0):
        return ("NAME",)
    if 32 + lrn + 4 * nc + (ls + 1) // 2 + ls > bs:
        return ("FIELDS",)
    if flag & 0x910:
        return ("FLAG",)
    if ls == 0:
        return ("EMPTY",)
    sq = p + 36 + lrn + 4 * nc
    ql = sq + (ls + 1) // 2
    if data[ql] == 0xFF:
        return ("NOQUAL",)
    name = data[p + 36:p + 36 + lrn]
    cut = min([len(name)] + [k for k in (name.find(b"\0"), name.find(b" "), name.find(b"\t")) if k >= 0])
    packed = np.frombuffer(data, dtype=np.uint8, count=(ls + 1) // 2, offset=sq)
    nib = np.empty(2 * len(packed), dtype=np.uint8)
    nib[0::2], nib[1::2] = packed >> 4, packed & 15
    seq = np.frombuffer(CODES.encode(), dtype=np.uint8)[nib[:ls]].tobytes()
    q = np.frombuffer(data, dtype=np.uint8, count=ls, offset=ql)
    qual = (np.minimum(q, 93) + 33).astype(np.uint8).tobytes()
    return ("ok", p + 4 + bs, bytes(name[:cut]), seq, qual)


def py_parse(data, at_start=True, at_eof=False, min_len=0):
    """dict: records [(name, seq, qual)] (kept), n_records, n_short, consumed, header_bytes, departed, reason, bad_at"""
    data = bytes(data)
    out = dict(records=[], n_records=0, n_short=0, consumed=0, header_bytes=0, departed=0, reason=0, bad_at=0)
    p = 0
    if len(data) == 0:
        return out
    if at_start:
        st, hb = py_header(data)
        if st == "bad":
            out.update(departed=1, reason=R["HEADER"])
            return out
        if st == "incomplete":
            if at_eof:
                out.update(departed=1, reason=R["TRUNCATED"])
            return out
        p = out["header_bytes"] = hb
    while p < len(data):
        r = py_record(data, p)
        if r[0] == "incomplete":
            if at_eof:
                out.update(departed=1, reason=R["TRUNCATED"], bad_at=p)
            break
        if r[0] != "ok":
            out.update(departed=1, reason=R[r[0]], bad_at=p)
            break
        p = r[1]
        out["n_records"] += 1
        if len(r[3]) < min_len:
            out["n_short"] += 1
        else:
            out["records"].append(r[2:])
    out["consumed"] = p
    return out


def same(res, want):
    """a FastqParse of bam_parse_host / Bgzf.bam_parse against py_parse's dict: every field, every array"""
    i = res.info
    recs = want["records"]
    assert res.guards_intact and res.untouched_beyond_results
    assert (i["n_records"], i["n_kept"], i["n_short"], i["consumed"], i["header_bytes"], i["departed"], i["reason"], i["bad_at"]) == \
        (want["n_records"], len(recs), want["n_short"], want["consumed"], want["header_bytes"], want["departed"], want["reason"], want["bad_at"]), (i, {k: v for k, v in want.items() if k != "records"})
    assert res.records() == recs
    assert i["name_bytes"] == sum(len(r[0]) for r in recs) and i["base_bytes"] == sum(len(r[1]) for r in recs)


# ---- corpora --------------------------------------------------------------------------------------------------------------
L_SEQS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257)


def _seq(rng, n):
    return "".join(CODES[int(c)] for c in rng.integers(0, 16, n))


def _qual(rng, n):
    q = rng.integers(0, 60, n).astype(np.uint8)
    if n >= 4:
        q[rng.integers(0, n, 4)] = (0, 93, 94, 254)
    return bytes(q)


def valid_records(seed=5):
    """[(args of record(), kwargs)]: every l_seq of L_SEQS with names of 1..9 and 254 bytes (the packed bases start at every
    alignment mod 8), a name with a blank, an empty name, n_cigar_op 0 and 2, flags 4 and 0x4D, qualities 0, 93, 94, 254, tags
    of 0..300 bytes, all 16 base codes"""
    rng = np.random.default_rng(seed)
    names = [bytes(rng.integers(ord("a"), ord("z") + 1, k).astype(np.uint8)) for k in list(range(1, 10)) + [254]] + [b"rd 7 x", b"tab\there", b""]
    out, k = [], 0
    for nc in (0, 2):
        for ls in L_SEQS:
            for _ in range(4 if nc == 0 else 1):
                name = names[k % len(names)]
                tags = tag_bytes((0, 8, 9, 37, 300, 0, 12, 123)[k % 8])
                out.append(((name, _seq(rng, ls), _qual(rng, ls)), dict(flag=(4, 0x4D)[k % 2], n_cigar=nc, tags=tags)))
                k += 1
    for nl in list(range(1, 10)) + [254]:                      # every name length with an odd and an even, long sequence
        out.append(((names[nl - 1 if nl < 10 else 9], _seq(rng, 64 + nl), _qual(rng, 64 + nl)), dict()))
    out.append(((b"codes", CODES + CODES[::-1] + "A", bytes(range(33))), dict()))
    return out


def build(recs, head=None):
    return (header() if head is None else head) + b"".join(record(*a, **kw) for a, kw in recs)


def valid_corpus():
    """[(name, data, at_start)]"""
    recs = valid_records()
    return [("all", build(recs), True), ("no_header", build(recs, b""), False), ("three", build(recs[:3]), True),
            ("header_alone", header(b"@HD\tVN:1.6\n"), True), ("empty", b"", True)]


def header_corpus():
    recs = valid_records()[:5]
    return [("plain", build(recs, header()), header()),
            ("refs3", build(recs, header(b"@HD\n", [(b"chr1", 1000), (b"c", 5), (b"a_longer_name", 1 << 30)])), None),
            ("text200000", build(recs, header(b"@CO\t" + b"x" * 199995 + b"\n")), None)]


def _edit(rec, at, fmt, value):
    b = bytearray(rec)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def bad_records():
    """[(reason, record bytes)]: one or more records per reason, each not strict for that reason alone or first"""
    good = record(b"victim", "ACGTACGTAC", bytes(range(20, 30)), tags=tag_bytes(20))
    return [("BLOCK", _edit(good, 0, "<I", 33)), ("BLOCK", _edit(good, 0, "<I", MAX_RECORD + 1)), ("BLOCK", _edit(good, 0, "<I", 0xFFFFFFFF)),
            ("BLOCK", _edit(good, 0, "<I", 0)),
            ("NAME", _edit(good, 12, "<B", 0)), ("NAME", _edit(good, 36 + 6, "<B", ord("x"))),
            ("FIELDS", _edit(good, 20, "<I", 0x7FFFFFFF)), ("FIELDS", _edit(good, 20, "<I", 0xFFFFFFFF)), ("FIELDS", _edit(good, 16, "<H", 0xFFFF)),
            ("FIELDS", _edit(good, 12, "<B", 255)),
            ("FLAG", _edit(good, 18, "<H", 0x10)), ("FLAG", _edit(good, 18, "<H", 0x104)), ("FLAG", _edit(good, 18, "<H", 0x800)),
            ("EMPTY", record(b"nobases", "", b"")), ("EMPTY", _edit(good, 20, "<I", 0)),
            ("NOQUAL", _edit(good, 36 + 7 + 5, "<B", 0xFF))]


def departure_corpus():
    """[(name, data, at_eof, reason, index of the bad record)]: every reason at the first, a middle and the last record"""
    recs = [record(*a, **kw) for a, kw in valid_records()[:6]]
    out = []
    for j, (why, bad) in enumerate(bad_records()):
        for where in (0, 3, 6):
            out.append(("%s%d@%d" % (why, j, where), header() + b"".join(recs[:where]) + bad + b"".join(recs[where:]), False, R[why], where))
    whole = header() + b"".join(recs)
    for where, cut in ((0, len(header()) + 2), (0, len(header()) + len(recs[0]) - 1),(3, len(header() + b"".join(recs[:3])) + 4), (5, len(whole) - 1)):
        out.append(("TRUNCATED@%d" % where, whole[:cut], True, R["TRUNCATED"], where))
    out.append(("HEADER_magic", b"BAM\2" + whole[4:], False, R["HEADER"], 0))
    out.append(("HEADER_l_text", whole[:4] + struct.pack("<i", -5) + whole[8:], False, R["HEADER"], 0))
    out.append(("HEADER_cut_eof", whole[:7], True, R["TRUNCATED"], 0))
    out.append(("HEADER_n_ref", whole[:8] + struct.pack("<i", MAX_REFS + 1) + whole[12:], False, R["HEADER"], 0))
    out.append(("HEADER_n_ref_eof", whole[:8] + struct.pack("<i", MAX_REFS) + whole[12:], True, R["TRUNCATED"], 0))   # more than the data holds
    return out


def cut_corpus():
    """a 3-record file and every prefix length of it"""
    data = build(valid_records()[:3])
    return data, range(len(data) + 1)


# ---- records placed against the tiles, and decoys -------------------------------------------------------------------------
def pad_to(prefix_len, rec_args, target):
    """record(*rec_args) with a tag that makes it end exactly at byte `target` of a file in which it begins at prefix_len"""
    bare = len(record(*rec_args))
    pad = target - prefix_len - bare
    assert pad == 0 or pad >= 8, pad
    return record(*rec_args, tags=tag_bytes(pad))


def tile_case(k):
    """data whose third record's fixed 36 bytes begin at TILE - k (k = 1..3 split block_size itself), and the records in it"""
    rng = np.random.default_rng(100 + k)
    recs = [(b"r%d" % i, _seq(rng, 30 + i), _qual(rng, 30 + i)) for i in range(5)]
    data = header() + record(*recs[0])
    data += pad_to(len(data), recs[1], TILE - k)
    assert len(data) == TILE - k
    data += b"".join(record(*r) for r in recs[2:])
    return data, recs


def fake_chain(n_fake, last_block=None):
    """n_fake self-consistent record images back to back (each plausible under every check of the rule); the last one's
    block_size can be set so that the chain ends at a chosen byte"""
    out = b""
    for i in range(n_fake):
        r = record(b"fake%d" % i, "ACGT" * 3, b"\x1e" * 12)
        if i == n_fake - 1 and last_block is not None:
            r = _edit(r, 0, "<I", last_block)
        out += r
    return out


def decoy_case(kind):
    """(data, records): a B:C tag whose bytes look like records.
    a: a chain of three fake records is the first plausible header of tile 1; the true next record starts later in that tile
    b: a 150 KB tag with such a chain at the start of every tile it covers
    c: a fake chain in tile 1 whose last record ends exactly on the true next record"""
    rng = np.random.default_rng(7)
    recs = [(b"r%d" % i, _seq(rng, 50 + i), _qual(rng, 50 + i)) for i in range(6)]
    data = header() + record(*recs[0])
    bare = record(*recs[1])
    tag_at = len(data) + len(bare) + 8                                  # file offset of the tag's first payload byte
    size = {"a": TILE + 3000, "b": 150000, "c": TILE + 3000}[kind]
    payload = bytearray(b"\xff" * size)
    end = tag_at + size                                                 # where the true next record starts
    for t in range(1, (end - 1) // TILE + 1):
        at = t * TILE - tag_at
        if at < 0:
            continue
        if kind == "c":
            two = fake_chain(2)
            last_start = t * TILE + len(two)
            chain = two + fake_chain(1, last_block=end - last_start - 4)[:60]
        else:
            chain = fake_chain(3)
        if at + len(chain) <= size:
            payload[at:at + len(chain)] = chain
    data += record(*recs[1], tags=b"XPBC" + struct.pack("<I", size) + bytes(payload))
    assert len(data) == end
    data += b"".join(record(*r) for r in recs[2:])
    return data, recs


def minimal_records(n, bad_at=None):
    """n records of minimal size (l_seq 2, 3-byte names), built with numpy; record bad_at gets flag 0x10"""
    one = np.frombuffer(record(b"abc", "AC", b"\x14\x15"), dtype=np.uint8)
    arr = np.tile(one, (n, 1))
    idx = np.arange(n)
    for j in range(3):                                                  # names from the index, base 26
        arr[:, 36 + j] = ord("a") + (idx // 26 ** j) % 26
    arr[:, 40] = ((idx % 15 + 1) << 4 | (idx // 15 % 15 + 1)).astype(np.uint8)
    if bad_at is not None:
        arr[bad_at, 18] = 0x10
    return header() + arr.tobytes(), len(one)
