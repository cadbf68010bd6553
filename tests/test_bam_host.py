"""The host side of BAM input (include/c3poa.h "Unaligned BAM records on the GPU"), no GPU: the host statement
c3_bam_parse_host against the tests' own statement of the rule (bam_cases.py_parse), and the reader on a .bam file against the
reader on the FASTQ text of the same records (bam_cases.fastq_of) -- the FASTQ route is the yardstick, equality is exact."""
import ctypes as C
import struct

import pytest

from c3poa_amd import _lib, synth
import bam_cases as B
import test_inflate_host as H


def host(data, **kw):
    return _lib.bam_parse_host(data, **kw)


# ---- the host statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.valid_corpus(), ids=lambda c: c[0])
def test_valid_corpus_equals_the_rule(case):
    _name, data, at_start = case
    for at_eof in (False, True):
        for min_len in (0, 9, 300):
            want = B.py_parse(data, at_start, at_eof, min_len)
            assert not want["departed"] and want["consumed"] == len(data)
            B.same(host(data, at_start=at_start, at_eof=at_eof, min_len=min_len), want)


def test_valid_corpus_holds_what_the_issue_lists():
    recs = B.valid_records()
    ls = {len(a[1]) for a, _k in recs}
    assert set(B.L_SEQS) <= ls
    assert {len(a[0]) for a, _k in recs} >= set(range(0, 10)) | {254}
    assert {(36 + len(a[0]) + 1 + 4 * k.get("n_cigar", 0)) % 8 for a, k in recs} == set(range(8))      # where the packed bases start
    assert {k.get("n_cigar", 0) for _a, k in recs} == {0, 2} and {k.get("flag", 4) for _a, k in recs} == {4, 0x4D}
    assert {0, 93, 94, 254} <= {q for a, _k in recs for q in a[2]}
    assert set("".join(a[1] for a, _k in recs)) == set(B.CODES)
    assert {0, 300} <= {len(k.get("tags", b"")) for _a, k in recs}
    want = B.py_parse(B.build(recs))["records"]
    assert want == [B.delivered(*a) for a, _k in recs]                   # the writer and the rule agree on what is delivered
    assert any(b" " in a[0] for a, _k in recs) and any(a[0] == b"" for a, _k in recs)


def test_every_cut_of_a_three_record_file():
    data, cuts = B.cut_corpus()
    full = B.py_parse(data)
    for n in cuts:
        for at_eof in (False, True):
            want = B.py_parse(data[:n], True, at_eof)
            res = host(data[:n], at_eof=at_eof)
            B.same(res, want)
            whole = [p for p in (0, full["header_bytes"], *_ends(data)) if p <= n]
            assert res.info["consumed"] == (whole[-1] if whole[-1] >= full["header_bytes"] else 0)
            assert res.info["departed"] == (1 if at_eof and 0 < n and res.info["consumed"] != n else 0)


def _ends(data):
    p, out = B.py_header(data)[1], []
    while p < len(data):
        p += 4 + struct.unpack_from("<I", data, p)[0]
        out.append(p)
    return out


@pytest.mark.parametrize("case", B.header_corpus(), ids=lambda c: c[0])
def test_headers(case):
    _name, data, _h = case
    want = B.py_parse(data)
    assert want["n_records"] == 5 and want["header_bytes"] > 0
    B.same(host(data), want)
    hb = want["header_bytes"]
    for n in (1, 3, 4, 7, 8, 11, 12, hb - 1, hb, hb + 1):                # a header that is merely incomplete: consumed = 0, no error
        res = host(data[:n])
        B.same(res, B.py_parse(data[:n]))
        assert res.info["consumed"] == (hb if n >= hb else 0) and not res.info["departed"]
    mid = data[hb:]
    B.same(host(mid, at_start=False), B.py_parse(mid, at_start=False))


@pytest.mark.parametrize("case", B.departure_corpus(), ids=lambda c: c[0])
def test_departures(case):
    _name, data, at_eof, reason, index = case
    for min_len in (0, 9):
        want = B.py_parse(data, True, at_eof, min_len)
        assert want["departed"] == 1 and want["reason"] == reason and want["n_records"] == index
        res = host(data, at_eof=at_eof, min_len=min_len)
        B.same(res, want)
        assert res.info["bad_at"] == res.info["consumed"]


def test_decoys_and_tiles_pass_the_host_statement_first():
    for kind in "abc":
        data, recs = B.decoy_case(kind)
        want = B.py_parse(data)
        assert want["records"] == [B.delivered(*r) for r in recs]
        B.same(host(data), want)
    for k in (0, 1, 3, 4, 35):
        data, recs = B.tile_case(k)
        assert _ends(data)[1] == B.TILE - k
        B.same(host(data), B.py_parse(data))


def test_capacity_and_arguments():
    data = B.build(B.valid_records()[:8])
    want = B.py_parse(data)
    nk = len(want["records"])
    nb, bb = sum(len(r[0]) for r in want["records"]), sum(len(r[1]) for r in want["records"])
    B.same(host(data, caps=(nb, bb, nk)), want)                          # exactly enough
    for caps in ((nb - 1, bb, nk), (nb, bb - 1, nk), (nb, bb, nk - 1), (0, 0, 0)):
        with pytest.raises(_lib.C3Error) as e:
            host(data, caps=caps)
        assert e.value.code == _lib.E_LIMIT and e.value.guards_intact and e.value.untouched
        assert (e.value.info["n_kept"], e.value.info["name_bytes"], e.value.info["base_bytes"]) == (nk, nb, bb)
    B.same(host(b""), B.py_parse(b""))                                    # n == 0 is success
    lib = _lib.load()
    info = _lib.BamInfo()
    buf = C.create_string_buffer(64)
    a = [buf, 8, 1, 0, 0, buf, 8, buf, buf, buf, 8, buf, 1, C.byref(info)]
    for k in (0, 5, 7, 8, 9, 11, 13):                                     # each pointer null in turn
        b = list(a)
        b[k] = None
        assert lib.c3_bam_parse_host(*b) == _lib.E_ARG
    for k, v in ((1, -1), (6, -1), (10, -1), (12, -1)):
        b = list(a)
        b[k] = v
        assert lib.c3_bam_parse_host(*b) == _lib.E_ARG
    b = list(a)
    b[1] = 0x7FF00001
    assert lib.c3_bam_parse_host(*b) == _lib.E_LIMIT                      # n > C3_FASTQ_MAX_TEXT, before a byte is read
    assert lib.c3_bam_parse(None, *a) == _lib.E_ARG                       # the device call: a null handle


# ---- the reader -------------------------------------------------------------------------------------------------------------
N_READS = 120
SETTINGS = ((1, 0, None), (7, 5000, 0), (1000, 0, None), (1000, 0, 0))   # tests/test_gpu_stage_device.py; None = the length cut


def _group(hb):
    nb, nn = int(hb.off[-1]), int(hb.name_off[-1])
    return (hb.n, hb.n_short, list(hb.name_off), list(hb.off), C.string_at(hb.c.names, nn) if nn else b"",
            C.string_at(hb.c.seqs, nb) if nb else b"", C.string_at(hb.c.quals, nb) if nb else b"")


def groups(path, max_reads, max_bases, min_len, **kw):
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    try:
        while True:
            out.append(_group(rd.next(max_reads, min_len, max_bases)))
            if out[-1][0] == 0:
                return out
    finally:
        rd.close()


def reader_records():
    """cfg2 reads with Phred values as BAM holds them, and a few records of the edge corpus in between"""
    recs = [(r[0].encode(), r[1], bytes(ord(c) - 33 for c in r[2])) for r in synth.generate("cfg2", n_reads=N_READS)]
    edge = [a for a, _k in B.valid_records() if a[0] and len(a[1]) > 2][:20]
    return recs[:50] + edge + recs[50:]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam")
    recs = reader_records()
    data = B.header(b"@HD\tVN:1.6\tSO:unsorted\n@PG\tID:basecaller\n") + b"".join(record_with_tags(i, r) for i, r in enumerate(recs))
    fq = str(d / "reads.fastq")
    open(fq, "wb").write(B.fastq_of(recs))
    bam = {}
    for block in (4096, 65280):
        bam[block] = str(d / ("reads%d.bam" % block))
        open(bam[block], "wb").write(H.bgzf_file(data, block=block))
    lens = sorted(len(r[1]) for r in recs)
    return dict(dir=d, recs=recs, data=data, fq=fq, bam=bam, cut=lens[len(lens) // 3])


def record_with_tags(i, r):
    return B.record(*r, flag=(4, 0x4D)[i % 2], tags=B.tag_bytes((0, 8, 45, 300)[i % 4]))


@pytest.mark.parametrize("block", [4096, 65280])
def test_reader_groups_equal_fastq_groups(corpus, block):
    for mr, mb, ml in SETTINGS:
        ml = corpus["cut"] if ml is None else ml
        want = groups(corpus["fq"], mr, mb, ml)
        assert groups(corpus["bam"][block], mr, mb, ml) == want, (block, mr, mb, ml)
        assert sum(g[0] + g[1] for g in want) == len(corpus["recs"])


def test_reader_names_only_noqual_and_reserved_bytes(corpus):
    rd, rf = _lib.Reader(corpus["bam"][4096], n_sets=2, names_only=True), _lib.Reader(corpus["fq"], n_sets=2, names_only=True)
    a, b = rd.next(1000), rf.next(1000)
    assert (a.n, list(a.name_off), list(a.off)) == (b.n, list(b.name_off), list(b.off))
    assert C.string_at(a.c.names, int(a.name_off[-1])) == C.string_at(b.c.names, int(b.name_off[-1]))
    assert rd.noqual() == 0
    rd.close(), rf.close()
    rd = _lib.Reader(corpus["bam"][4096], n_sets=3)
    rd.next(1000)
    assert rd.noqual() == 0 and 0 < rd.reserved_bytes() <= 16 * 3 * (1 << 20) + 32 * len(corpus["data"])      # sized by the file, not by max_reads
    rd.close()


def test_reader_error_text_at_a_departure(corpus, tmp_path):
    recs = corpus["recs"][:10]
    good = [B.record(*r) for r in recs]
    bad = B.record(b"rev", "ACGT", b"\x10" * 4, flag=0x10)
    data = B.header() + b"".join(good[:7]) + bad + b"".join(good[7:])
    at = len(B.header() + b"".join(good[:7]))
    for block in (4096, 65280):
        p = str(tmp_path / ("dep%d.bam" % block))
        open(p, "wb").write(H.bgzf_file(data, block=block))
        rd = _lib.Reader(p, n_sets=1)
        assert rd.next(5).n == 5                                          # the groups of earlier calls are delivered as usual
        with pytest.raises(ValueError) as e:
            rd.next(5)                                                    # records 5 and 6 of this call are dropped with the error
        msg = str(e.value)
        assert "record 7 " in msg and "inflated byte %d:" % at in msg and "samtools fastq" in msg, msg
        rd.close()
    p = str(tmp_path / "cut.bam")                                        # the file ends inside a record
    open(p, "wb").write(H.bgzf_file(data[:at + 20], block=4096))
    rd = _lib.Reader(p, n_sets=1)
    with pytest.raises(ValueError) as e:
        rd.next(100)
    assert "record 7 " in str(e.value) and "inflated byte %d:" % at in str(e.value) and "ends inside a record" in str(e.value)
    rd.close()


def test_reader_refuses_what_is_not_bam(corpus, tmp_path, monkeypatch):
    p = str(tmp_path / "plain.bam")                                      # a .bam that is not BGZF
    open(p, "wb").write(corpus["data"])
    rd = _lib.Reader(p)
    with pytest.raises(ValueError) as e:
        rd.next(10)
    assert "not a BGZF file" in str(e.value)
    rd.close()
    p = str(tmp_path / "text.bam")                                       # BGZF, but FASTQ text inside
    open(p, "wb").write(H.bgzf_file(B.fastq_of(corpus["recs"][:5])))
    rd = _lib.Reader(p)
    with pytest.raises(ValueError) as e:
        rd.next(10)
    assert "record 0 at inflated byte 0:" in str(e.value) and "not a BAM header" in str(e.value)
    rd.close()
    monkeypatch.setenv("C3_NO_BGZF", "1")                                 # no escape for a .bam: it is BGZF by definition
    assert groups(corpus["bam"][4096], 1000, 0, 0) == groups(corpus["fq"], 1000, 0, 0)
    monkeypatch.delenv("C3_NO_BGZF")
    with pytest.raises(OSError):                                          # a byte range on a .bam
        _lib.Reader(corpus["bam"][4096], byte_range=(0, -1))
    r = C.c_void_p()
    assert _lib.load().c3_reader_open_range(corpus["bam"][4096].encode(), 1, 0, -1, C.byref(r)) == _lib.E_ARG


def test_reader_damaged_member_keeps_its_text(corpus, tmp_path):
    raw = bytearray(open(corpus["bam"][4096], "rb").read())
    raw[len(raw) // 2] ^= 0x55
    p = str(tmp_path / "damaged.bam")
    open(p, "wb").write(bytes(raw))
    rd = _lib.Reader(p, n_sets=1)
    with pytest.raises(ValueError) as e:
        while rd.next(1000).n:
            pass
    assert "BGZF input: a member is damaged" in str(e.value)
    rd.close()


def test_blat_finder_refuses_bam(tmp_path):
    """--splint-finder blat writes blat's FASTA with the text reader, which does not read BAM: a clear message, no blat run"""
    import types
    from c3poa_amd import preprocess
    bam = tmp_path / "reads.bam"
    bam.write_bytes(H.bgzf_file(B.build(B.valid_records()[:2])))
    args = types.SimpleNamespace(reads=str(bam), splint_finder="blat", lencutoff=0, splint_file="none.fasta")
    with pytest.raises(RuntimeError, match="--splint-finder blat reads FASTQ only"):
        preprocess.ensure_psl("blat", args, str(tmp_path) + "/")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["reads.bam"]
