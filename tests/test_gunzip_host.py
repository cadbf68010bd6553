"""gzip input without a GPU: c3_gunzip_host -- find, decode with markers, chain, windows and resolve by plain
loops, the procedure and decoder that c3_gunzip runs on the device -- against Python's zlib and gzip on everything RFC 1952
allows, at piece sizes that put seams everywhere, and on damage.  tests/test_gpu_gunzip.py runs the same cases on the device."""
import ctypes as C
import functools
import gzip
import zlib

import numpy as np
import pytest

from c3poa_amd import _lib, synth

PIECES = (64, 1024, 32768)


# ---- the reference: zlib's gzip decoder, member after member (gzread's rule) ---------------------------------------------
def reference(data):
    """the text zlib delivers, or None where it raises or the file ends inside a member"""
    out = []
    while data:
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data))
        except zlib.error:
            return None
        if not d.eof:
            return None
        data = d.unused_data
    return b"".join(out)


def gz(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    if not sync_every:
        return c.compress(text) + c.flush()
    parts = []
    for at in range(0, len(text), sync_every):
        parts.append(c.compress(text[at:at + sync_every]))
        parts.append(c.flush(zlib.Z_SYNC_FLUSH))
    return b"".join(parts) + c.flush()


def with_header(member, extra=None, name=None, comment=None, hcrc=False):
    """the member with FEXTRA / FNAME / FCOMMENT / FHCRC fields put into its header"""
    assert member[:4] == b"\x1f\x8b\x08\x00"
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = bytearray(member[:10])
    h[3] = flg
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += (zlib.crc32(bytes(h)) & 0xFFFF).to_bytes(2, "little")
    return bytes(h) + member[10:]


@functools.lru_cache(maxsize=None)
def fastq_text(n_reads=60):
    return "".join("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]) for r in synth.generate("cfg2", n_reads=n_reads)).encode()


# ---- hand-made deflate streams (the helpers of tests/test_gpu_inflate.py's host file, for blocks that are not final) ------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):                      # k bits of v, least significant first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):                     # a Huffman code: most significant bit first
        self.put(int(bin(c)[2:].zfill(k)[::-1], 2) if k else 0, k)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 0xFF]) if self.n else b"")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6                   # a complete code-length code
LIT_LENS = [8] * 226 + [9] * 60                # complete: 226 / 256 + 60 / 512 = 1
DIST_LENS = [4] * 2 + [5] * 28                 # complete: 2 / 16 + 28 / 32 = 1


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


LIT, DIST, CL = canon(LIT_LENS), canon(DIST_LENS), canon(CL_LENS)


def dynamic_block(b, tokens, final):
    """one dynamic block appended to the bit writer.  tokens: ints (literals) and (length, distance) pairs"""
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(LIT_LENS) - 257, 5)
    b.put(len(DIST_LENS) - 1, 5)
    b.put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(CL_LENS[s], 3)
    for v in LIT_LENS + DIST_LENS:
        b.code(*CL[v])
    for t in tokens:
        if isinstance(t, tuple):
            s = 28 if t[0] == 258 else max(i for i in range(28) if LBASE[i] <= t[0])
            b.code(*LIT[257 + s])
            b.put(t[0] - LBASE[s], LEXT[s])
            s = max(i for i in range(30) if DBASE[i] <= t[1])
            b.code(*DIST[s])
            b.put(t[1] - DBASE[s], DEXT[s])
        else:
            b.code(*LIT[t])
    b.code(*LIT[256])


def expand(blocks):
    out = bytearray()
    for tokens in blocks:
        for t in tokens:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    out.append(out[-t[1]])
            else:
                out.append(t)
    return bytes(out)


def handmade(blocks, text=None):
    """a gzip member of dynamic blocks; text: what the trailer says it holds (default: what the tokens give)"""
    b = Bits()
    for k, tokens in enumerate(blocks):
        dynamic_block(b, tokens, k == len(blocks) - 1)
    text = expand(blocks) if text is None else text
    return b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + b.bytes() + zlib.crc32(text).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")


def _lits(rng, n):
    return [int(x) for x in rng.integers(0, 256, n)]


def far_match_streams():
    """a first block of 40 000 random literals (more than 32 KiB compressed), then a block whose matches reach back into it:
    at the larger piece sizes the second block starts a piece of its own and its sources lie in the piece before"""
    rng = np.random.default_rng(5)
    first = _lits(rng, 40000)
    out = []
    for D in (1, 2, 32767, 32768):
        for L in (3, 258):
            out.append(("far D=%d L=%d" % (D, L), handmade([first, [(L, D), 7, 200, (258, D)] + _lits(rng, 50), _lits(rng, 30)])))
    return out


def copied_line_stream():
    """a 300-byte line carried forward by matches through four blocks of 6 KB each (pieces shorter than 32 KiB): every block
    copies the line from the block before (markers), copies its own copy again (markers copied by a match), and the last
    one reaches back over two blocks (a window composed from two pieces)"""
    rng = np.random.default_rng(6)
    line = _lits(rng, 300)
    blocks = [line + _lits(rng, 5700)]
    for k in range(1, 5):
        back = 6100 if k == 1 else 6000                      # the line stands at 0 in block 0, at 100 in the others
        toks = _lits(rng, 100) + [(258, back), (42, back)] + _lits(rng, 50) + [(258, 350), (42, 350)]
        toks += _lits(rng, 6000 - 100 - 300 - 50 - 300)
        if k == 4:
            toks += [(200, 2 * 6000 + 37), (258, 3 * 6000 + 11)]
        blocks.append(toks)
    return handmade(blocks)


def decoy_file():
    """level-0 gzip of a level-6 .gz file: the stored blocks carry real dynamic block headers that are no block starts"""
    return gz(gz(fastq_text()), level=0)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """(name, file, environment) of every file that must inflate to what zlib delivers"""
    fq = fastq_text()
    small = fq[:60000]
    cases = [("level %d" % lv, gz(fq, lv), {}) for lv in (1, 6, 9)]
    cases += [("memLevel %d" % m, gz(fq[:100000] if m == 1 else fq, 6, m), {}) for m in (1, 8)]
    cases.append(("Z_FIXED", gz(small, 6, 8, zlib.Z_FIXED), {}))
    cases.append(("level 0", gz(small, 0), {}))
    cases.append(("sync flush every 1000", gz(small, 6, 8, sync_every=1000), {}))
    hdr = with_header(gz(small), extra=b"XY\x03\x00abc", name=b"reads.fastq", comment=b"made by hand", hcrc=True)
    cases.append(("FEXTRA FNAME FCOMMENT FHCRC", hdr, {}))
    cases.append(("FNAME alone", with_header(gz(small), name=b"r.fq"), {}))
    three = gz(fq[:70000]) + gz(b"") + with_header(gz(fq[70000:150000], 9), extra=b"\0" * 300, name=b"second")
    cases.append(("three members, one empty", three, {}))
    cut = len(gz(fq[:70000])) + len(gz(b"")) + 150             # a stretch boundary inside the third member's FEXTRA field
    cases.append(("stretch boundary inside a member header (the call holds the whole file: only the cut is exercised)", three, {"C3_GUNZIP_STRETCH": str(cut)}))
    cases.append(("stretches of 5000 bytes", gz(fq, 6), {"C3_GUNZIP_STRETCH": "5000"}))
    cases += [(n, d, {}) for n, d in far_match_streams()]
    cases.append(("line copied through four pieces", copied_line_stream(), {}))
    cases.append(("decoy", decoy_file(), {}))
    cases.append(("slab cap 3000", gz(small), {"C3_GUNZIP_SLAB": "3000"}))
    cases.append(("slab cap 3000, small blocks", gz(small, 6, 1), {"C3_GUNZIP_SLAB": "3000"}))
    cases.append(("relaunch cap 0", decoy_file(), {"C3_GUNZIP_RELAUNCH": "0"}))
    cases.append(("windows and resolve three pieces at a time", gz(small, 6, 1), {"C3_GUNZIP_FINISH": "3"}))
    cases.append(("the copied line, one piece at a time", copied_line_stream(), {"C3_GUNZIP_FINISH": "1"}))
    return cases


def damaged_cases():
    """(name, file) of damaged files; zlib's verdict is the reference (a flip in a header byte zlib does not look at is fine)"""
    fq = fastq_text()
    good = gz(fq[:50000])
    hdr = with_header(gz(fq[:20000]), extra=b"AB\x02\x00xy", name=b"n", hcrc=True)
    cases = []

    def flip(name, data, at, x=0x55):
        b = bytearray(data)
        b[at] ^= x
        cases.append(("%s, byte %d" % (name, at), bytes(b)))

    for at in (10, 11, 200, len(good) // 2, len(good) - 30, len(good) - 9):
        flip("deflate data", good, at)
    for at in range(len(good) - 8, len(good) - 4):
        flip("CRC", good, at)
    for at in range(len(good) - 4, len(good)):
        flip("ISIZE", good, at)
    for at in range(0, 10):
        flip("header", good, at, 0x01)
        flip("header", good, at, 0xE0)
    for at in range(10, 22):
        flip("header fields", hdr, at)
    two = good + gz(fq[50000:60000])
    flip("second member's header", two, len(good) + 1)
    flip("second member's data", two, len(good) + 40)
    cases.append(("garbage behind the member", good + b"\0\0\0\0"))
    cases.append(("a second member without its trailer", two[:-8]))
    rng = np.random.default_rng(8)
    first = _lits(rng, 300)
    cases.append(("distance in front of the member, first block", handmade([first[:100] + [(3, 101)] + first[100:]], b"")))
    cases.append(("distance in front of the member, second block", handmade([first, [(258, 32768), 1, 2]], b"")))
    cases.append(("distance in front of the member by one", handmade([first, [(3, 301), 1, 2]], b"")))
    return cases


def truncations():
    data = gz(fastq_text()[:3000])
    return [("cut at %d" % at, data[:at]) for at in range(0, len(data), 10)]


def host_verdict(data, piece, env, monkeypatch):
    """(text or None, error code or 0, stats) of c3_gunzip_host"""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        try:
            return _lib.gunzip_host(data, piece), 0, _lib.gunzip_stats()
        except _lib.C3Error as e:
            assert str(e).startswith("c3 error %d: c3_gunzip_host: " % e.code), str(e)
            return None, e.code, None


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", PIECES)
def test_valid_files_inflate_to_what_zlib_delivers(piece, monkeypatch):
    for name, data, env in valid_cases():
        want = reference(data)
        assert want is not None and want == gzip.decompress(data), name
        got, code, st = host_verdict(data, piece, env, monkeypatch)
        assert code == 0 and got == want, (name, piece, code)
        assert st["candidates"] == st["accepted"] + st["rejected"] and st["pieces"] >= 1, (name, piece, st)


def test_zlibs_own_dynamic_output_never_needs_the_fallback(monkeypatch):
    """the condition of DESIGN.md 5.14: single-member dynamic files made by zlib, at the default piece size and thresholds:
    no byte goes through the serial fallback, and every piece with a candidate is accepted or counted as rejected"""
    monkeypatch.delenv("C3_GUNZIP_PIECE", raising=False)
    fq = fastq_text()
    assert 200000 <= len(fq) <= 600000, len(fq)
    for lv in (1, 6, 9):
        for mem in (1, 8):
            data = gz(fq, lv, mem)
            got, code, st = host_verdict(data, 0, {}, monkeypatch)
            assert code == 0 and got == fq, (lv, mem)
            assert st["fallback_bytes"] == 0 and st["candidates"] >= 1, (lv, mem, st)
            assert st["candidates"] == st["accepted"] + st["rejected"], (lv, mem, st)
    st = host_verdict(gz(fq[:100000], 6, 1), 64, {}, monkeypatch)[2]
    assert st["candidates"] >= 200 and st["fallback_bytes"] == 0, st          # memLevel 1: a block every 128 symbols


def test_stats_tell_what_happened(monkeypatch):
    fq = fastq_text()
    st = host_verdict(gz(fq[:60000], 6, 8, zlib.Z_FIXED), 1024, {}, monkeypatch)[2]
    assert st["candidates"] == 0 and st["fallback_bytes"] == 60000 and st["relaunches"] == 0, st    # no candidate: the fallback, whole
    st = host_verdict(decoy_file(), 1024, {}, monkeypatch)[2]
    assert st["rejected"] >= 3 and st["accepted"] == 0 and st["relaunches"] >= 1 and st["fallback_bytes"] == 0, st
    got, code, st = host_verdict(decoy_file(), 1024, {"C3_GUNZIP_RELAUNCH": "0"}, monkeypatch)
    assert code == 0 and got == gz(fq) and st["relaunches"] == 0 and st["fallback_bytes"] > 0, st
    got, code, st = host_verdict(gz(fq[:60000]), 1024, {"C3_GUNZIP_SLAB": "3000"}, monkeypatch)
    assert code == 0 and got == fq[:60000] and st["full_slabs"] >= 1, st
    got, code, st = host_verdict(gz(fq[:60000], 6, 1), 1024, {"C3_GUNZIP_SLAB": "3000"}, monkeypatch)       # blocks that fit: partly taken
    assert code == 0 and got == fq[:60000] and st["full_slabs"] >= 1 and st["relaunches"] >= 1 and st["accepted"] >= 1, st
    got, code, st = host_verdict(gz(fq), 1024, {"C3_GUNZIP_STRETCH": "5000"}, monkeypatch)
    assert code == 0 and got == fq and st["stretches"] >= 10, st
    for name, data in far_match_streams():
        st = host_verdict(data, 32768, {}, monkeypatch)[2]
        assert st["accepted"] >= 1 and st["fallback_bytes"] == 0, (name, st)   # the block with the far matches began a piece
    st = host_verdict(copied_line_stream(), 1024, {}, monkeypatch)[2]
    assert st["accepted"] >= 3 and st["fallback_bytes"] == 0, st


@pytest.mark.parametrize("piece", PIECES)
def test_damaged_files_get_zlibs_verdict(piece, monkeypatch):
    n_bad = 0
    for name, data in damaged_cases() + truncations():
        want = reference(data)
        got, code, _st = host_verdict(data, piece, {}, monkeypatch)
        if want is None:
            assert code == _lib.E_DATA and got is None, (name, piece, code)
            n_bad += 1
        else:
            assert code == 0 and got == want, (name, piece, code)
    assert n_bad >= 40


def test_a_damaged_member_is_named(monkeypatch):
    fq = fastq_text()
    a, b = gz(fq[:30000]), gz(fq[30000:50000])
    bad = bytearray(a + b)
    bad[len(a) + len(b) - 6] ^= 1                                          # the second member's CRC
    with pytest.raises(_lib.C3Error) as e:
        _lib.gunzip_host(bytes(bad), 1024)
    assert e.value.code == _lib.E_DATA and "member 1 at offset %d is damaged (CRC)" % len(a) in str(e.value), str(e.value)
    with pytest.raises(_lib.C3Error) as e:
        _lib.gunzip_host(handmade([[1, 2, 3, (3, 4)]], b""), 64)
    assert "distance beyond the output so far" in str(e.value), str(e.value)


def test_arguments():
    lib = _lib.load()
    text = fastq_text()[:5000]
    data = gz(text)
    out, olen = C.create_string_buffer(len(text)), C.c_int64(-1)
    assert lib.c3_gunzip_host(data, len(data), out, len(text), C.byref(olen), 0) == 0 and out.raw == text and olen.value == len(text)
    assert lib.c3_gunzip_host(data, len(data), out, len(text) - 1, C.byref(olen), 0) == _lib.E_ARG          # cap one byte short
    assert "cap < inflated size" in lib.c3_last_error(None).decode()
    assert lib.c3_gunzip_host(None, len(data), out, len(text), C.byref(olen), 0) == _lib.E_ARG
    assert lib.c3_gunzip_host(data, len(data), None, len(text), C.byref(olen), 0) == _lib.E_ARG
    assert lib.c3_gunzip_host(data, len(data), out, len(text), None, 0) == _lib.E_ARG
    assert lib.c3_gunzip_host(data, -1, out, len(text), C.byref(olen), 0) == _lib.E_ARG
    assert lib.c3_gunzip_host(data, 0, out, len(text), C.byref(olen), 0) == 0 and olen.value == 0              # n == 0
    assert lib.c3_gunzip_host(None, 0, None, 0, C.byref(olen), 0) == 0 and olen.value == 0
    two = data + gz(text[:100])                                             # the first member alone is beyond cap: found on the way
    assert lib.c3_gunzip_host(two, len(two), out, len(text), C.byref(olen), 0) == _lib.E_ARG
    assert lib.c3_gunzip(None, data, len(data), out, len(text), C.byref(olen)) == _lib.E_ARG                   # null handle
    assert lib.c3_gunzip_stats(None, 8) == _lib.E_ARG
    assert _lib.gunzip_host(b"") == b"" and _lib.gunzip_host(gz(b"")) == b""
    assert set(_lib.gunzip_stats()) == set(_lib.GUNZIP_STATS)
    assert _lib._PROTOTYPES["c3_gunzip_host"][1][-1] is C.c_int64 and "c3_gunzip" in _lib.EXPORTS and "c3_gunzip_stats" in _lib.EXPORTS
