"""BGZF output of --bgzf: the host statement c3_bgzf_compress_host against the frozen format -- round trip
through gzip and raw inflate member by member, header fields, BSIZE, CRC, ISIZE, block cuts, the stored rule, and the
optimality of every dynamic code against an independent package-merge optimum.  CPU only."""
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

from c3poa_amd import _lib, synth

BLOCK = 65280
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _fastq_text(n_reads, cfg="cfg1", start=0):
    return "".join("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]) for r in synth.generate(cfg, n_reads=n_reads, start=start)).encode()


def _fasta_text(n_reads):
    return "".join(">%s_%d\n%s\n" % (r[0], len(r[1]), r[4]) for r in synth.generate("cfg1", n_reads=n_reads)).encode()


def _fib_block():
    """counts f(2..22) of the Fibonacci sequence (1, 2, 3, 5, ...; with the end-of-block's 1): plain Huffman codes reach
    21 bits, so the limit of 15 binds"""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    b = bytearray()
    for i, c in enumerate(f[1:]):
        b += bytes([65 + i]) * c
    random.Random(5).shuffle(b)
    return bytes(b)


def inputs():
    """name -> bytes: the inputs of the host test (and of the GPU test, which adds a large one)"""
    fq = _fastq_text(60)
    rnd = np.random.default_rng(7)
    return {
        "empty": b"",
        "one": b"@",
        "block-1": fq[:BLOCK - 1],
        "block": fq[:BLOCK],
        "block+1": fq[:BLOCK + 1],
        "repeat": b"A" * 150000,
        "all256": bytes(range(256)) * 700,
        "random": rnd.integers(0, 256, 3 * BLOCK + 17, dtype=np.uint8).tobytes(),
        "limit": _fib_block(),
        "fastq": fq,
        "fasta": _fasta_text(200),
    }


class _BitReader:
    def __init__(self, data):
        self.v, self.n, self.pos = int.from_bytes(data, "little"), 8 * len(data), 0

    def get(self, k):
        x = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return x

    def sym(self, table):
        """canonical decode: table = {(length, code): symbol}"""
        code, ln = 0, 0
        while True:
            code = (code << 1) | self.get(1)
            ln += 1
            if (ln, code) in table:
                return table[(ln, code)]
            assert ln <= 15


def _canon(lengths):
    bl = [0] * 16
    for x in lengths:
        bl[x] += 1
    bl[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + bl[b - 1]) << 1
        nxt[b] = c
    t = {}
    for s, x in enumerate(lengths):
        if x:
            t[(x, nxt[x])] = s
            nxt[x] += 1
    return t


def parse_dynamic(deflate):
    """the header of a dynamic block of this format: (literal lengths[257], code-length lengths[19], hclen, header bits)"""
    r = _BitReader(deflate)
    assert r.get(1) == 1 and r.get(2) == 2
    hlit, hdist, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    assert (hlit, hdist) == (257, 1)
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = r.get(3)
    assert hclen == 4 or cl[CL_ORDER[hclen - 1]] != 0, "HCLEN not trimmed"
    t = _canon(cl)
    lens = [r.sym(t) for _ in range(258)]
    assert max(lens) <= 15, "repeat codes are not used"
    assert lens[257] == 1, "the one distance code has length 1"
    return lens[:257], cl, hclen, r.pos


def pm_cost(weights, limit):
    """optimal total cost of a code with lengths <= limit (package-merge, boundary form): sum of the 2n - 2 cheapest items"""
    ws = sorted(weights)
    n = len(ws)
    if n == 1:
        return ws[0]
    items = list(ws)
    for _ in range(limit - 1):
        pk = [items[2 * i] + items[2 * i + 1] for i in range(len(items) // 2)]
        items = sorted(ws + pk)
    return sum(items[:2 * n - 2])


def pm_lengths(counts, limit):
    """the frozen procedure of DESIGN.md 5.3 in Python: leaves by (count, symbol), leaf before package on equal weight"""
    leaves = sorted((c, s) for s, c in counts.items() if c)
    n = len(leaves)
    if n == 1:
        return {leaves[0][1]: 1}
    cap, w = 2 * n - 2, [c for c, _ in leaves]
    prev, flags = w, {}
    for k in range(2, limit + 1):
        pk = [prev[2 * j] + prev[2 * j + 1] for j in range(len(prev) // 2)]
        merged, i, j = [], 0, 0
        while len(merged) < cap and (i < n or j < len(pk)):
            if i < n and (j >= len(pk) or w[i] <= pk[j]):
                merged.append((w[i], True)); i += 1
            else:
                merged.append((pk[j], False)); j += 1
        flags[k], prev = [f for _, f in merged], [x for x, _ in merged]
    depth, m = [0] * n, cap
    for k in range(limit, 1, -1):
        a = sum(flags[k][:m])
        for i in range(a):
            depth[i] += 1
        m = 2 * (m - a)
    for i in range(m):
        depth[i] += 1
    return {s: depth[i] for i, (_, s) in enumerate(leaves)}


def model_dynamic_bits(block):
    """exact bit count of the dynamic block the format prescribes for `block`"""
    cnt = np.bincount(np.frombuffer(block, dtype=np.uint8), minlength=256).tolist() + [1]
    lit = pm_lengths(dict(enumerate(cnt)), 15)
    lens = [lit.get(s, 0) for s in range(257)]
    clc = [0] * 19
    for x in lens + [1]:
        clc[x] += 1
    clm = pm_lengths(dict(enumerate(clc)), 7)
    cll = [clm.get(v, 0) for v in range(19)]
    hclen = 19
    while hclen > 4 and cll[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    return 3 + 14 + 3 * hclen + sum(clc[v] * cll[v] for v in range(19)) + sum(c * l for c, l in zip(cnt, lens)), lens


def check_members(data, out):
    """every member of `out` against the format; returns the number of stored members"""
    pos, k, n_stored = 0, 0, 0
    while pos < len(out):
        hdr = out[pos:pos + 18]
        assert hdr[:4] == b"\x1f\x8b\x08\x04" and hdr[4:8] == b"\0\0\0\0" and hdr[8] == 0 and hdr[9] == 255
        xlen, si1, si2, slen, bsize = struct.unpack("<HBBHH", hdr[10:18])
        assert (xlen, si1, si2, slen) == (6, 66, 67, 2)
        size = bsize + 1
        assert size <= 65536 and size <= 65311 and pos + size <= len(out)
        block = data[k * BLOCK:(k + 1) * BLOCK]
        assert len(block) == (BLOCK if (k + 1) * BLOCK <= len(data) else len(data) - k * BLOCK) and block
        deflate = out[pos + 18:pos + size - 8]
        crc, isize = struct.unpack("<II", out[pos + size - 8:pos + size])
        assert crc == zlib.crc32(block) and isize == len(block)
        d = zlib.decompressobj(-15)
        assert d.decompress(deflate) == block and d.eof and d.unused_data == b""
        dyn_bits, lens = model_dynamic_bits(block)
        stored_bits = 3 + 5 + 32 + 8 * len(block)
        if deflate[0] & 7 == 1:                                  # BFINAL 1, BTYPE 00
            n_stored += 1
            assert dyn_bits >= stored_bits
            assert deflate[1:5] == struct.pack("<HH", len(block), len(block) ^ 0xFFFF) and len(deflate) == 5 + len(block)
        else:
            assert dyn_bits < stored_bits
            plens, cl, hclen, hbits = parse_dynamic(deflate)
            assert plens == lens, "literal lengths differ from the procedure of DESIGN.md 5.3"
            cnt = np.bincount(np.frombuffer(block, dtype=np.uint8), minlength=256).tolist() + [1]
            used = [c for c in cnt if c]
            assert sum(c * l for c, l in zip(cnt, plens)) == pm_cost(used, 15), "literal code not optimal"
            assert sum(2.0 ** -x for x in plens if x) == 1.0 and max(plens) <= 15
            assert all((c > 0) == (x > 0) for c, x in zip(cnt, plens))
            clc = [0] * 19
            for x in plens + [1]:
                clc[x] += 1
            assert sum(clc[v] * cl[v] for v in range(19)) == pm_cost([c for c in clc if c], 7), "code-length code not optimal"
            assert max(cl) <= 7
            assert len(deflate) == (dyn_bits + 7) // 8
        pos += size
        k += 1
    assert k == (len(data) + BLOCK - 1) // BLOCK
    return n_stored


@pytest.mark.parametrize("name", list(inputs()))
def test_host_format(name):
    data = inputs()[name]
    out = _lib.bgzf_compress_host(data)
    assert gzip.decompress(out + _lib.BGZF_EOF) == data
    assert gzip.decompress(out) == data
    ns = check_members(data, out)
    if name == "random":
        assert ns == 4                                       # uniform bytes: every member stored
    elif name in ("fastq", "fasta", "repeat", "limit"):
        assert ns == 0
    if name == "limit":
        cnt = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).tolist() + [1]
        assert pm_cost([c for c in cnt if c], 15) > pm_cost([c for c in cnt if c], 30)      # the limit binds here
    assert len(out) <= _lib.load().c3_bgzf_bound(len(data))


def test_host_ratio_fastq_fasta():
    fq, fa = _fastq_text(200), _fasta_text(200)
    assert len(fq) / len(_lib.bgzf_compress_host(fq)) > 1.8
    assert len(fa) / len(_lib.bgzf_compress_host(fa)) > 3.0


def test_eof_member():
    assert len(_lib.BGZF_EOF) == 28 and gzip.decompress(_lib.BGZF_EOF) == b""
    assert struct.unpack("<H", _lib.BGZF_EOF[16:18])[0] == 27


def test_bound_and_refusals():
    lib = _lib.load()
    assert lib.c3_bgzf_bound(0) == 0 and lib.c3_bgzf_bound(1) == 65311 and lib.c3_bgzf_bound(BLOCK + 1) == 2 * 65311
    import ctypes as C
    out = C.create_string_buffer(65311)
    olen = C.c_int64(0)
    assert lib.c3_bgzf_compress_host(b"x" * 10, 10, out, 65310, C.byref(olen)) == -3       # cap < bound
    assert lib.c3_bgzf_compress_host(None, 10, out, 65311, C.byref(olen)) == -3
    assert lib.c3_bgzf_compress_host(b"x" * 10, 10, out, 65311, None) == -3
    assert lib.c3_bgzf_compress_host(b"x" * 10, 10, out, 65311, C.byref(olen)) == 0 and olen.value > 0


def test_cli_flag():
    import C3POa
    a = C3POa.parse_args(["-r", "x.fq", "-s", "s.fa"])
    assert a.bgzf is False and a.compress_output is False
    b = C3POa.parse_args(["-r", "x.fq", "-s", "s.fa", "--bgzf"])
    assert b.bgzf is True and b.compress_output is True
    c = C3POa.parse_args(["-r", "x.fq", "-s", "s.fa", "-co"])
    assert c.bgzf is False and c.compress_output is True
