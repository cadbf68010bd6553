"""BGZF input without a GPU: c3_bgzf_scan and c3_bgzf_decompress_host -- the decoder of c3_inflate.h that
k_inflate runs as well -- against Python's zlib through the contract of include/c3poa.h "BGZF input":

    hdr = 12 + XLEN;  payload = member[hdr : size - 8];  crc, isize = trailer
    d = zlib.decompressobj(-15);  out = d.decompress(payload, 65537)
    accepted  <=>  d.eof and len(out) == isize and isize <= 65536 and zlib.crc32(out) == crc

The corpus builders here are imported by tests/test_gpu_inflate.py, which puts the same bytes through the kernel."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from c3poa_amd import _lib, synth

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


# ---- the reference --------------------------------------------------------------------------------------------------
def split_members(data):
    """the members of a well-framed buffer (the tests' own walk: BC subfield anywhere in the extra field)"""
    out, at = [], 0
    while at < len(data):
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        q, size = at + 12, None
        while q + 4 <= at + 12 + xlen:
            slen = struct.unpack_from("<H", data, q + 2)[0]
            if data[q:q + 2] == b"BC" and slen == 2:
                size = struct.unpack_from("<H", data, q + 4)[0] + 1
                break
            q += 4 + slen
        assert size is not None and at + size <= len(data)
        out.append(bytes(data[at:at + size]))
        at += size
    return out


def ref_member(member):
    """the contract: the member's bytes, or None when it is not accepted"""
    xlen = struct.unpack_from("<H", member, 10)[0]
    payload = member[12 + xlen:len(member) - 8]
    crc, isize = struct.unpack_from("<II", member, len(member) - 8)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, 65537)
    except zlib.error:
        return None
    if d.eof and len(out) == isize and isize <= 65536 and zlib.crc32(out) == crc:
        return out
    return None


def ours(fn, data):
    """fn(data), or None when it refuses with C3_E_DATA (anything else is a failure of the test)"""
    try:
        return fn(data)
    except _lib.C3Error as e:
        assert e.code == _lib.E_DATA, e
        assert "member" in str(e)
        return None


# ---- members made with zlib in the bgzip layout ---------------------------------------------------------------------------
def wrap(payload, text, extra_first=False):
    xtra = (b"XY" + struct.pack("<H", 3) + b"abc") if extra_first else b""
    xlen = 6 + len(xtra)
    total = 12 + xlen + len(payload) + 8
    assert total <= 65536
    return (struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + xtra + b"BC" + struct.pack("<HH", 2, total - 1)
            + payload + struct.pack("<II", zlib.crc32(text), len(text)))


def bgzf_members(text, block=BLOCK, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush=False, extra_first=False):
    out = []
    for i in range(0, len(text), block):
        chunk = text[i:i + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        if full_flush:
            h = len(chunk) // 2
            comp = co.compress(chunk[:h]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(chunk[h:]) + co.flush()
        else:
            comp = co.compress(chunk) + co.flush()
        out.append(wrap(comp, chunk, extra_first))
    return out


def bgzf_file(text, **kw):
    return b"".join(bgzf_members(text, **kw)) + EOF_MEMBER


def fastq_text(n_reads=40):
    return "".join("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]) for r in synth.generate("cfg2", n_reads=n_reads)).encode()


# ---- hand-made members: a bit writer, fixed-Huffman tokens, dynamic headers ---------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):                      # k bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):                     # a Huffman code: most significant bit first
        for b in range(k - 1, -1, -1):
            self.put((c >> b) & 1, 1)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_sym(length):
    s = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
    return s, length - LBASE[s]


def dist_sym(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, dist - DBASE[s]


def canon(lens):
    """RFC 1951 3.2.2: symbol -> (code, length)"""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, v in enumerate(lens):
            if v == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)


def put_tokens(b, tokens, lit, dist):
    """tokens: ints (literals) and (length, distance) pairs; lit / dist: symbol -> (code, length); then end-of-block"""
    for t in tokens:
        if isinstance(t, tuple):
            s, x = len_sym(t[0])
            b.code(*lit[257 + s])
            b.put(x, LEXT[s])
            s, x = dist_sym(t[1])
            b.code(*dist[s])
            b.put(x, DEXT[s])
        else:
            b.code(*lit[t])
    b.code(*lit[256])


def fixed_member(tokens):
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    put_tokens(b, tokens, FIXED_LIT, {s: (s, 5) for s in range(30)})
    return b.bytes()


def far_match_members():
    """zlib's compressor never emits a distance above 32 506: 32 768 random literals, a match (L, D), two literals, a match
    (258, D), for the distances around the lane count and at the format's limit"""
    rng = np.random.default_rng(11)
    lits = [int(x) for x in rng.integers(0, 256, 32768)]
    out = []
    for D in (1, 2, 3, 63, 64, 65, 32767, 32768):
        for L in (3, 4, 64, 65, 258):
            out.append(("far D=%d L=%d" % (D, L), fixed_member(lits + [(L, D), 7, 200, (258, D)])))
    return out


# code-length code of the hand-made dynamic headers: complete (13 codes of 4 bits, 6 of 5)
CL_LENS = [4] * 13 + [5] * 6


def dynamic_member(lit_lens, dist_lens, tokens, cl_lens=None, clseq=None, hlit=None, body_lit=None, body_dist=None):
    """one final dynamic block.  clseq: the (code-length symbol, extra value) sequence; default = every length written out.
    hlit: the HLIT field when it is not len(lit_lens) - 257.  body_lit / body_dist: the code lengths the tokens are written
    with, where the declared sets cannot write them."""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(cl_lens[s], 3)
    cl = canon(cl_lens)
    if clseq is None:
        clseq = [(v, 0) for v in list(lit_lens) + list(dist_lens)]
    for s, x in clseq:
        b.code(*cl[s])
        b.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    lit = canon(lit_lens if body_lit is None else body_lit)
    put_tokens(b, tokens, lit, canon(dist_lens if body_dist is None else body_dist))
    return b.bytes()


def _lits(**kw):
    v = [0] * kw.pop("n", 258)
    for k, ln in kw.items():
        v[int(k[1:])] = ln
    return v


def dynamic_header_members():
    A, B = 65, 66
    four = _lits(s65=2, s66=2, s256=2, s257=2)                   # A, B, end-of-block, length 3: complete
    out = [
        ("one distance code of length 1", dynamic_member(four, [1], [A, B, A, (3, 1), B])),
        ("no distance code, literals only", dynamic_member(four, [0], [A, B, B, A])),
        ("no distance code, a match", dynamic_member(four, [0], [A, B, (3, 1)], body_dist=[1])),
        ("over-subscribed literal/length set", dynamic_member(_lits(s65=1, s66=1, s256=1), [1], [], body_lit=four)),
        ("incomplete literal/length set", dynamic_member(_lits(s65=2, s66=2, s256=2), [1], [A, B])),
        ("a single literal/length code of length 1", dynamic_member(_lits(s256=1), [1], [])),
        ("incomplete code-length code", dynamic_member(four, [1], [A, B], cl_lens=[4] * 13 + [5] * 5 + [0])),
        ("no end-of-block code", dynamic_member(_lits(s65=1, s66=1), [1], [A, B], body_lit=four)),
        ("repeat code 16 first", dynamic_member(four, [1], [A], clseq=[(16, 0)] + [(0, 0)] * 62 + [(2, 0), (2, 0)] + [(0, 0)] * 189
                                                + [(2, 0), (2, 0), (1, 0)])),
        ("a repeat that runs past the end", dynamic_member(four, [1], [A], clseq=[(0, 0)] * 65 + [(2, 0), (2, 0)] + [(18, 127)] + [(18, 40)]
                                                           + [(2, 0), (2, 0), (18, 127)])),
        ("valid repeats 16 17 18", dynamic_member(_lits(s65=3, s66=3, s67=3, s68=3, s256=2, s257=2), [1], [A, 67, 68, (3, 1), B, (3, 1)],
                                                  clseq=[(18, 54), (3, 0), (16, 0), (18, 127), (17, 7), (18, 28), (2, 0), (2, 0), (1, 0)])),
        ("HLIT = 30", dynamic_member(_lits(n=287, s65=2, s66=2, s256=2, s257=2), [1], [A], hlit=30)),
        ("HLIT = 31", dynamic_member(_lits(n=288, s65=2, s66=2, s256=2, s257=2), [1], [A], hlit=31)),
    ]
    return out


def handmade_member(payload):
    """the payload wrapped with the trailer of what zlib makes of it (of sixteen bytes where zlib refuses it, so that the
    decoder gets as far as the stream's own fault)"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload, 65537)
        if not d.eof:
            text = b"?" * 16
    except zlib.error:
        text = b"?" * 16
    return wrap(payload, text[:65536])


# ---- the corpora ------------------------------------------------------------------------------------------------------
def valid_corpus():
    """(name, file bytes, text): every file is made of accepted members and ends with the end-of-file member"""
    fq = fastq_text()
    rnd = np.random.default_rng(5).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    texts = [("fastq", fq), ("random", rnd), ("A", b"A" * 300000), ("empty", b""), ("one", b"x"),
             ("65280", fq[:65280]), ("65281", fq[:65281])]
    out = []
    for tn, text in texts:
        for vn, kw in [("l0", dict(level=0)), ("l1", dict(level=1)), ("l6", dict(level=6)), ("l9", dict(level=9)),
                       ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman", dict(strategy=zlib.Z_HUFFMAN_ONLY)),
                       ("rle", dict(strategy=zlib.Z_RLE)), ("fullflush", dict(full_flush=True))]:
            out.append(("%s %s" % (tn, vn), bgzf_file(text, **kw), text))
    out.append(("fastq block 301", bgzf_file(fq, block=301), fq))
    out.append(("fastq block 4096", bgzf_file(fq, block=4096), fq))
    out.append(("fastq foreign subfield", bgzf_file(fq, extra_first=True), fq))
    out.append(("fastq block 4096 foreign subfield", bgzf_file(fq, block=4096, extra_first=True), fq))
    for tn, text in (("fastq", fq), ("random", rnd)):
        out.append(("k_bgzf format %s" % tn, _lib.bgzf_compress_host(text) + EOF_MEMBER, text))
    for name, payload in far_match_members():
        m = handmade_member(payload)
        text = ref_member(m)
        assert text is not None and len(text) == 32768 + 2 + 258 + int(name.split("L=")[1]), name      # zlib accepts all forty
        out.append((name, m + EOF_MEMBER, text))
    return out


def damaged_corpus():
    """(name, member): single-byte flips at positions >= 18 and truncated payloads of five members, one seed"""
    fq = fastq_text()
    far = dict(far_match_members())
    bases = [("dynamic", bgzf_members(fq)[0]), ("fixed", bgzf_members(fq, strategy=zlib.Z_FIXED)[0]),
             ("stored", bgzf_members(fq, level=0)[0]), ("literal-only", split_members(_lib.bgzf_compress_host(fq))[0]),
             ("long matches", handmade_member(far["far D=32768 L=258"]))]
    rng = np.random.default_rng(20240)
    out = []
    for bn, m in bases:
        assert ref_member(m) is not None
        for k in range(200):
            pos = int(rng.integers(18, len(m)))
            bad = bytearray(m)
            bad[pos] ^= int(rng.integers(1, 256))
            out.append(("%s flip %d at %d" % (bn, k, pos), bytes(bad)))
        for cut in (1, 2, 100):
            payload = m[18:-8][:-cut]
            total = 18 + len(payload) + 8
            out.append(("%s cut %d" % (bn, cut), m[:16] + struct.pack("<H", total - 1) + payload + m[-8:]))
    return out


def framing_cases():
    m = bgzf_members(fastq_text(8))[0]
    big = bytearray(m)
    big[-4:] = struct.pack("<I", 65537)
    magic = bytearray(m)
    magic[1] ^= 0x10
    return [("flipped magic byte", bytes(magic) + EOF_MEMBER),
            ("BSIZE smaller than the header", m[:16] + struct.pack("<H", 10) + m[18:] + EOF_MEMBER),
            ("BSIZE beyond the buffer", m[:16] + struct.pack("<H", len(m) + 40) + m[18:]),
            ("ISIZE > 65536", bytes(big) + EOF_MEMBER),
            ("buffer ends inside a member", m + m[:len(m) // 2])]


def check_verdicts(fn, cases):
    """every case: the same verdict as the reference, the same bytes where both accept; returns (accepted, refused)"""
    acc = 0
    for name, m in cases:
        want, got = ref_member(m), ours(fn, m)
        assert (want is None) == (got is None), (name, "zlib accepts" if want is not None else "zlib refuses")
        if want is not None:
            assert got == want, name
            acc += 1
    return acc, len(cases) - acc


# ---- the tests -----------------------------------------------------------------------------------------------------------
def test_valid_corpus_inflates_to_its_text():
    corpus = valid_corpus()
    assert len(corpus) == 7 * 8 + 4 + 2 + 40
    for name, data, text in corpus:
        members = split_members(data)
        assert all(len(m) <= 65536 for m in members), name
        assert b"".join(ref_member(m) for m in members) == text, name          # the reference itself accepts the file
        assert _lib.bgzf_scan(data) == (len(members), len(text)), name
        assert _lib.bgzf_decompress_host(data) == text, name
    assert _lib.bgzf_scan(corpus[3 * 8][1]) == (1, 0)                          # the empty text: the end-of-file member alone


def test_handmade_dynamic_headers_get_zlibs_verdict():
    cases = [(n, handmade_member(p)) for n, p in dynamic_header_members()]
    acc, ref = check_verdicts(_lib.bgzf_decompress_host, cases)
    verdict = {n: ref_member(m) is not None for n, m in cases}
    # (zlib decides; these four are what RFC 1951 and zlib's table builder leave no doubt about)
    assert verdict["one distance code of length 1"] and verdict["no distance code, literals only"] and verdict["valid repeats 16 17 18"]
    assert not verdict["over-subscribed literal/length set"] and not verdict["repeat code 16 first"]
    assert acc >= 3 and ref >= 2


def test_damaged_members_get_zlibs_verdict():
    cases = damaged_corpus()
    assert len(cases) == 5 * 203
    acc, ref = check_verdicts(_lib.bgzf_decompress_host, cases)
    assert ref > 900                                                            # nearly every flip is caught by the stream or the CRC


def test_damage_inside_a_file_names_the_member():
    fq = fastq_text()
    ms = bgzf_members(fq, block=4096)
    bad = bytearray(ms[5])
    bad[len(bad) // 2] ^= 0x55
    assert ref_member(bytes(bad)) is None
    with pytest.raises(_lib.C3Error) as e:
        _lib.bgzf_decompress_host(b"".join(ms[:5]) + bytes(bad) + b"".join(ms[6:]) + EOF_MEMBER)
    assert e.value.code == _lib.E_DATA and "member 5 " in str(e.value)


def test_framing_errors_are_data_errors():
    for name, data in framing_cases():
        for fn in (_lib.bgzf_scan, _lib.bgzf_decompress_host):
            with pytest.raises(_lib.C3Error) as e:
                fn(data)
            assert e.value.code == _lib.E_DATA, name


def test_arguments():
    lib = _lib.load()
    text = fastq_text(8)
    data = bgzf_file(text)
    n, olen, nm, ob = len(data), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    out = C.create_string_buffer(len(text))
    assert lib.c3_bgzf_decompress_host(data, n, out, len(text), C.byref(olen)) == 0 and out.raw == text and olen.value == len(text)
    assert lib.c3_bgzf_decompress_host(data, n, out, len(text) - 1, C.byref(olen)) == _lib.E_ARG         # cap one byte short
    assert lib.c3_bgzf_decompress_host(None, n, out, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress_host(data, n, None, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress_host(data, n, out, len(text), None) == _lib.E_ARG
    assert lib.c3_bgzf_decompress_host(data, 0, out, len(text), C.byref(olen)) == 0 and olen.value == 0   # n == 0
    assert lib.c3_bgzf_decompress_host(None, 0, None, 0, C.byref(olen)) == 0 and olen.value == 0
    assert lib.c3_bgzf_scan(None, n, C.byref(nm), C.byref(ob)) == _lib.E_ARG
    assert lib.c3_bgzf_scan(data, 0, C.byref(nm), C.byref(ob)) == 0 and (nm.value, ob.value) == (0, 0)
    assert lib.c3_bgzf_decompress(None, data, n, out, len(text), C.byref(olen)) == _lib.E_ARG             # null handle
    assert _lib.bgzf_decompress_host(b"") == b"" and _lib.bgzf_scan(b"") == (0, 0)


def test_inflate_flag():
    import C3POa
    base = ["-r", "x", "-s", "y"]
    assert C3POa.parse_args(base).inflate == "host"
    assert C3POa.parse_args(base + ["--inflate", "gpu"]).inflate == "gpu"
    assert C3POa.parse_args(base + ["--inflate", "host"]).inflate == "host"
    with pytest.raises(SystemExit):
        C3POa.parse_args(base + ["--inflate", "zlib"])
