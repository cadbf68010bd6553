"""-r reads.bam on the GPU (k_bam; include/c3poa.h "Unaligned BAM records on the GPU"): Bgzf.bam_parse against
the host statement on the corpora of tests/bam_cases.py (the data at every offset of a dword), at lane, workgroup and tile
boundaries, over decoys that look like records, with guard bytes round every output array; the native reader with the device
parser on a .bam against the reader of the plain FASTQ of the same records (the yardstick: the FASTQ route); errors; and the
command line against the run on the plain FASTQ.  Equality is exact everywhere."""
import ctypes as C

import numpy as np
import pytest

from c3poa_amd import _lib, synth
import bam_cases as B
import test_bam_host as T
import test_inflate_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    zz = _lib.Bgzf(0)
    yield zz
    zz.close()


def same(dev, host, what):
    assert dev.info == host.info, (what, dev.info, host.info)
    assert dev.names == host.names and dev.seqs == host.seqs and dev.quals == host.quals, what
    assert list(dev.name_off) == list(host.name_off) and list(dev.off) == list(host.off), what
    assert dev.guards_intact and dev.untouched_beyond_results, what


def both(z, data, at_start=True, at_eof=False, min_len=0, what="", offsets=(0,)):
    """device == host statement, field for field (reason and bad_at included); returns the host result"""
    host = _lib.bam_parse_host(data, at_start, at_eof, min_len)
    for off in offsets:
        same(z.bam_parse(data, at_start, at_eof, min_len, text_offset=off), host, "%s (offset %d)" % (what, off))
    return host


# ---- the stand-alone call -----------------------------------------------------------------------------------------------
def test_corpora_at_every_offset(z):
    for name, data, at_start in B.valid_corpus():
        for min_len in (0, 9):
            host = both(z, data, at_start, False, min_len, name, offsets=(0, 1, 2, 3))
            assert host.info["consumed"] == len(data) and not host.info["departed"]
    for name, data, _h in B.header_corpus():
        assert both(z, data, what=name, offsets=(0, 1, 2, 3)).info["n_records"] == 5
    data, cuts = B.cut_corpus()
    for n in cuts:
        for at_eof in (False, True):
            both(z, data[:n], True, at_eof, 0, "cut at %d, at_eof %d" % (n, at_eof), offsets=(0, 1, 2, 3))
    for name, data, at_eof, reason, index in B.departure_corpus():
        host = both(z, data, True, at_eof, 0, name, offsets=(0, 1, 2, 3))
        assert (host.info["departed"], host.info["reason"], host.info["n_records"]) == (1, reason, index), name


def _drawn(n_records, seed):
    rng = np.random.default_rng(seed)
    pool = list(range(1, 10)) + [63, 64, 65, 255, 256, 257]
    recs = []
    for i in range(n_records):
        ls = int(rng.choice(pool))
        recs.append(B.record(b"d%d c" % i, B._seq(rng, ls), B._qual(rng, ls), tags=B.tag_bytes((0, 8, 21)[i % 3])))
    return B.header() + b"".join(recs)


def test_lane_and_workgroup_boundaries(z):
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        data = _drawn(n, n)
        host = both(z, data, what="%d records" % n, offsets=(0, 3))
        assert host.info["n_kept"] == n and host.info["consumed"] == len(data)
        both(z, data[:-1], True, True, 4, "%d records, min_len, the last one cut at the end of the file" % n)
        both(z, data[:-1], True, False, 0, "%d records, last one cut" % n)
    B.same(z.bam_parse(_drawn(257, 5)), B.py_parse(_drawn(257, 5)))         # ... and once against the tests' own parser


@pytest.mark.parametrize("k", range(36))
def test_a_record_header_across_a_tile_boundary(z, k):
    data, recs = B.tile_case(k)
    host = both(z, data, what="fixed fields at TILE - %d" % k)
    assert host.records() == [B.delivered(*r) for r in recs]
    both(z, data[:B.TILE + 10], True, True, 0, "... and the file cut behind the boundary")


def test_long_records_leave_tiles_without_a_start(z):
    rng = np.random.default_rng(11)
    recs = [(b"long%d" % i, B._seq(rng, n), B._qual(rng, n)) for i, n in enumerate([70000, 32768, 200000, 32769, 5, 32767, 70001])]
    data = B.header() + b"".join(B.record(*r) for r in recs)
    host = both(z, data, what="70 000 and 200 000 bases", offsets=(0, 1))
    assert host.records() == [B.delivered(*r) for r in recs]
    both(z, data, True, False, 32769, "long records, min_len")


def test_far_more_records_than_tiles(z):
    data, size = B.minimal_records(75000)
    assert 3_000_000 < len(data) < 3_500_000
    host = both(z, data, what="75 000 minimal records", offsets=(0, 1))
    assert host.info["n_kept"] == 75000 and host.info["consumed"] == len(data)
    assert host.records()[70000] == B.py_record(data, len(B.header()) + 70000 * size)[2:]
    bad, _ = B.minimal_records(75000, bad_at=50001)                          # a departure far into the scans
    host = both(z, bad, what="75 000 minimal records, record 50 001 reverse-strand")
    assert host.info["departed"] == 1 and host.info["n_kept"] == 50001 and host.info["reason"] == B.R["FLAG"]
    # handle reuse: a second, smaller call on the same handle; then a third call, after a C3_E_LIMIT
    both(z, data[:len(B.header()) + 7 * size + 13], what="second call, smaller")
    with pytest.raises(_lib.C3Error) as e:
        z.bam_parse(data, caps=(3 * 75000, 2 * 75000, 74999))
    assert e.value.code == _lib.E_LIMIT and e.value.info["n_kept"] == 75000 and e.value.guards_intact and e.value.untouched
    both(z, B.cut_corpus()[0], True, True, 0, "third call")


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_decoys_do_not_change_the_serial_walk(z, kind):
    data, recs = B.decoy_case(kind)
    want = B.py_parse(data)
    assert want["records"] == [B.delivered(*r) for r in recs]
    B.same(_lib.bam_parse_host(data), want)                                  # through the host statement on the CPU first
    host = both(z, data, what="decoy " + kind, offsets=(0, 2))
    assert host.records() == want["records"]


def test_capacity_and_arguments(z):
    data = B.build(B.valid_records()[:8])
    need = _lib.bam_parse_host(data).info
    caps = (need["name_bytes"], need["base_bytes"], need["n_kept"])
    same(z.bam_parse(data, caps=caps), _lib.bam_parse_host(data), "exactly enough")
    for k in range(3):
        c = list(caps)
        c[k] -= 1
        with pytest.raises(_lib.C3Error) as e:
            z.bam_parse(data, caps=tuple(c))
        assert e.value.code == _lib.E_LIMIT and e.value.info == need and e.value.guards_intact and e.value.untouched, c
    same(z.bam_parse(b""), _lib.bam_parse_host(b""), "n == 0")
    same(z.bam_parse(data), _lib.bam_parse_host(data), "the handle works afterwards")


# ---- the reader ---------------------------------------------------------------------------------------------------------
def _groups(path, max_reads, max_bases, min_len, **kw):
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    try:
        while True:
            out.append(T._group(rd.next(max_reads, min_len, max_bases)))
            if out[-1][0] == 0:
                return out, rd.parse_stats()
    finally:
        rd.close()


DEV = dict(inflate_device=0, parse_device=True)


@pytest.fixture(scope="module")
def want(corpus):
    got = {}

    def ref(mr, mb, ml):
        if (mr, mb, ml) not in got:
            got[(mr, mb, ml)] = T.groups(corpus["fq"], mr, mb, ml)           # the plain-FASTQ reader: computed once, left unchanged
        return got[(mr, mb, ml)]
    return ref


corpus = T.corpus


@pytest.mark.parametrize("stretch", [1, 3, 4096])
@pytest.mark.parametrize("block", [4096, 65280])
def test_reader_equals_fastq_reader(corpus, want, monkeypatch, block, stretch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
    n = len(corpus["recs"])
    for mr, mb, ml in T.SETTINGS:
        ml = corpus["cut"] if ml is None else ml
        got, stats = _groups(corpus["bam"][block], mr, mb, ml, **DEV)
        assert got == want(mr, mb, ml), (block, stretch, mr, mb, ml)
        assert stats[1] == 0 and stats[2] == n and stats[0] >= 1, (block, stretch, stats)        # every stretch on the device
    if block == 4096:
        n_members = -(-len(corpus["data"]) // block)
        assert _groups(corpus["bam"][block], 1000, 0, 0, **DEV)[1][0] == -(-n_members // stretch)
    got, stats = _groups(corpus["bam"][block], 1000, 0, 0, inflate_device=0)                     # k_inflate, host statement
    assert got == want(1000, 0, 0) and stats == (0, 0, 0)


def test_reader_long_header_and_long_read_one_member_per_stretch(corpus, tmp_path, monkeypatch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", "1")
    rng = np.random.default_rng(2)
    recs = corpus["recs"][:6] + [(b"long", B._seq(rng, 70000), B._qual(rng, 70000))] + corpus["recs"][6:12]
    data = B.header(b"@CO\t" + b"x" * 199995 + b"\n") + b"".join(B.record(*r) for r in recs)
    fq, bam = str(tmp_path / "l.fastq"), str(tmp_path / "l.bam")
    open(fq, "wb").write(B.fastq_of(recs))
    open(bam, "wb").write(H.bgzf_file(data, block=65280))
    for mr, mb, ml in ((1000, 0, 0), (3, 0, 0)):
        got, stats = _groups(bam, mr, mb, ml, **DEV)
        assert got == T.groups(fq, mr, mb, ml)
        assert stats[1] == 0 and stats[2] == len(recs) and stats[0] == -(-len(data) // 65280)


def test_reader_names_only(corpus, monkeypatch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", "3")
    a = _lib.Reader(corpus["bam"][4096], n_sets=1, names_only=True, **DEV)
    b = _lib.Reader(corpus["fq"], n_sets=1, names_only=True)
    ga, gb = a.next(1000), b.next(1000)
    assert (ga.n, list(ga.name_off), list(ga.off)) == (gb.n, list(gb.name_off), list(gb.off))
    assert C.string_at(ga.c.names, int(ga.name_off[-1])) == C.string_at(gb.c.names, int(gb.name_off[-1]))
    assert a.parse_stats()[1] == 0 and a.noqual() == 0
    a.close(), b.close()


def test_reader_device_groups(corpus, want, monkeypatch):
    """stage_device=True: the device bytes copied back equal the FASTQ reader's bytes, with 0 host bytes"""
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", "3")
    _lib.load()
    rt = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln))
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rd = _lib.Reader(corpus["bam"][4096], n_sets=1, stage_device=True, **DEV)
    got = []
    while True:
        hb = rd.next(60, 0, 0)
        nb, nn = int(hb.off[-1]), int(hb.name_off[-1])
        if hb.n:
            assert hb.dev is not None and not hb.c.seqs and hb.dev.bytes == nb
            sq, ql = C.create_string_buffer(nb), C.create_string_buffer(nb)
            assert rt.hipMemcpy(sq, hb.dev.d_seqs, nb, 2) == 0 and rt.hipMemcpy(ql, hb.dev.d_quals, nb, 2) == 0
            got.append((hb.n, hb.n_short, list(hb.name_off), list(hb.off), C.string_at(hb.c.names, nn), sq.raw[:nb], ql.raw[:nb]))
        else:
            got.append((0, hb.n_short, [0], [0], b"", b"", b""))
            break
    stage = rd.stage_stats()
    rd.close()
    assert got == want(60, 0, 0)
    assert stage == (len(got) - 1, 0, 0), stage


def test_reader_errors_equal_the_host_path(corpus, tmp_path, monkeypatch):
    recs = corpus["recs"][:10]
    good = [B.record(*r) for r in recs]
    bad = B.record(b"rev", "ACGT", b"\x10" * 4, flag=0x10)
    data = B.header() + b"".join(good[:7]) + bad + b"".join(good[7:])
    for name, blob in (("dep.bam", data), ("cut.bam", data[:len(data) - 9]), ("nohdr.bam", data[:7])):
        p = str(tmp_path / name)
        open(p, "wb").write(H.bgzf_file(blob, block=4096))
        for stretch in (1, 4096):
            monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
            texts = []
            for kw in ({}, DEV):
                rd = _lib.Reader(p, n_sets=1, **kw)
                with pytest.raises(ValueError) as e:
                    while rd.next(5).n:
                        pass
                texts.append(str(e.value))
                rd.close()
            assert texts[0] == texts[1] and "BAM input: record " in texts[0], texts
    raw = bytearray(open(corpus["bam"][4096], "rb").read())                  # a damaged member fails with the text it always had
    raw[len(raw) // 2] ^= 0x55
    p = str(tmp_path / "damaged.bam")
    open(p, "wb").write(bytes(raw))
    texts = []
    for kw in (dict(inflate_device=0), DEV):
        with pytest.raises(ValueError) as e:
            _groups(p, 7, 0, 0, **kw)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "damaged" in texts[0], texts


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_cli_bam_equals_fastq(tmp_path, capfd, monkeypatch):
    import test_gpu_inflate as G
    monkeypatch.setenv("C3_STREAM_STATS", "1")
    recs = list(synth.generate("cfg2", n_reads=48))
    plain, _text = G._run_cli(tmp_path / "a", recs)
    want = G._outputs(plain)
    assert set(want) >= {"c3poa.log"} | {"Splint1/" + f for f in G.FILES} and len(want["Splint1/R2C2_Consensus.fasta"]) > 1000
    data = B.header(b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(
        B.record(r[0].encode(), r[1], bytes(ord(c) - 33 for c in r[2]), tags=B.tag_bytes((0, 19)[i % 2])) for i, r in enumerate(recs))
    bam = ("reads.bam", H.bgzf_file(data))
    assert G._outputs(G._run_cli(tmp_path / "b", recs, reads=bam)[0]) == want
    assert G._outputs(G._run_cli(tmp_path / "c", recs, ["--inflate", "gpu"], reads=bam)[0]) == want
    capfd.readouterr()
    got = G._run_cli(tmp_path / "d", recs, ["--inflate", "gpu", "--parse", "gpu"], reads=bam)[0]
    err = capfd.readouterr().err
    assert G._outputs(got) == want
    assert "parse_stretches_host=0 " in err + " " and "parse_records_device=%d" % len(recs) in err and "parse_stretches_device=1" in err
    gz = G._run_cli(tmp_path / "e", recs, ["--inflate", "gpu", "--parse", "gpu", "--emit", "gpu", "--bgzf"], reads=bam)[0]
    assert G._outputs(gz, gz=True) == want
