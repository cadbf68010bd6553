"""--parse gpu (k_fastq): Bgzf.fastq_parse against the host statement on the corpora of tests/test_fastq_host.py (the text at
every offset of a dword), at lane, workgroup, tile and scan boundaries, with guard bytes round every output array; the
native reader with the device parser against the reader of the plain file (groups equal, nothing parsed on the host); the
fallback to the host parser at a departure; errors; and the command line against the run on the plain FASTQ."""
import ctypes as C
import gzip

import numpy as np
import pytest

from c3poa_amd import _lib
import test_fastq_host as F
import test_inflate_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    zz = _lib.Bgzf(0)
    yield zz
    zz.close()


def both(z, text, at_eof=False, min_len=0, what="", offsets=(0,)):
    """device == host statement, field for field; returns the host result"""
    host = _lib.fastq_parse_host(text, at_eof, min_len)
    for off in offsets:
        dev = z.fastq_parse(text, at_eof, min_len, text_offset=off)
        F.same(dev, host, "%s (offset %d)" % (what, off))
        assert dev.guards_intact and dev.untouched_beyond_results, what
    return host


# ---- the stand-alone call -----------------------------------------------------------------------------------------------
def test_corpora_at_every_offset(z):
    for name, text, at_eof, min_len in F.valid_corpus() + F.cut_corpus():
        both(z, text, at_eof, min_len, name, offsets=(0, 1, 2, 3))
    for name, text, at_eof, start, n_before in F.departure_corpus():
        host = both(z, text, at_eof, 0, name, offsets=(0, 1, 2, 3))
        assert host.info["departed"] == 1 and host.info["consumed"] == start and host.info["n_records"] == n_before, name


def _drawn(n_records, seed):
    rng = np.random.default_rng(seed)
    pool = list(range(1, 10)) + [63, 64, 65, 255, 256, 257]
    return b"".join(F.rec(b"d%d c" % i, int(rng.choice(pool)), seed=i) for i in range(n_records))


def test_lane_and_workgroup_boundaries(z):
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        text = _drawn(n, n)
        host = both(z, text, False, 0, "%d records" % n, offsets=(0, 3))
        assert host.info["n_kept"] == n and host.info["consumed"] == len(text)
        both(z, text[:-1], True, 4, "%d records, min_len, no last newline" % n)
        both(z, text[:-1], False, 0, "%d records, last one cut" % n)
    F.check(z.fastq_parse(_drawn(257, 5)), _drawn(257, 5))                 # ... and once against the tests' own parser


def test_tile_and_scan_boundaries(z):
    # records that span two 64 KiB tiles (and take the workgroup's path of the gather), and the lengths either side of it
    long_ = b"".join(F.rec(b"long%d" % i, n, seed=i) for i, n in enumerate([70000, 32768, 70001, 32769, 5, 32767, 70000]))
    host = both(z, long_, False, 0, "70 000-base records", offsets=(0, 1))
    assert host.info["n_kept"] == 7
    F.check(z.fastq_parse(long_, text_offset=2), long_)
    both(z, long_, False, 32769, "70 000-base records, min_len")
    # about 3 MB of 40-byte records: many '\n' per lane, far more records than tiles
    rng = np.random.default_rng(3)
    seqs = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (75000, 14))
    quals = rng.integers(35, 74, (75000, 14), dtype=np.uint8)
    small = b"".join(b"@r%05d\n%s\n+\n%s\n" % (i, seqs[i].tobytes(), quals[i].tobytes()) for i in range(75000))
    assert len(small) == 40 * 75000
    host = both(z, small, False, 0, "40-byte records", offsets=(0, 1))
    assert host.info["n_kept"] == 75000 and host.info["consumed"] == len(small)
    F.check(z.fastq_parse(small, True), small, True)
    bad = small[:40 * 50001] + b"\n" + small[40 * 50001:]                  # a departure far into the scans
    host = both(z, bad, False, 0, "40-byte records with a blank line")
    assert host.info["departed"] == 1 and host.info["n_kept"] == 50001
    # a second call on the same handle with a smaller text: nothing of the earlier one shows
    both(z, small[:40 * 7 + 13], False, 0, "second call, smaller")
    both(z, F.THREE, True, 0, "third call")


def test_capacity_and_arguments(z):
    text = b"".join(F.rec(b"n%d" % i, n) for i, n in enumerate([10, 20, 30]))
    need = _lib.fastq_parse_host(text).info
    F.check(z.fastq_parse(text, caps=(6, 60, 3)), text)
    for caps in ((5, 60, 3), (6, 59, 3), (6, 60, 2)):
        with pytest.raises(_lib.C3Error) as e:
            z.fastq_parse(text, caps=caps)
        assert e.value.code == _lib.E_LIMIT and e.value.info == need and e.value.guards_intact and e.value.untouched, caps
    lib = _lib.load()
    args, info = F._raw_args(text)
    assert lib.c3_fastq_parse(z.z, *args) == 0 and info.n_kept == 3
    for k in (0, 4, 6, 7, 8, 10, 12):
        bad = list(args)
        bad[k] = None
        assert lib.c3_fastq_parse(z.z, *bad) == _lib.E_ARG, k
    empty = list(args)
    empty[0], empty[1] = None, 0
    assert lib.c3_fastq_parse(z.z, *empty) == 0 and info.n_records == 0 and info.consumed == 0
    F.check(z.fastq_parse(text), text)                                      # the handle works afterwards


# ---- the reader ---------------------------------------------------------------------------------------------------------
def _groups(path, max_reads, max_bases, min_len, **kw):
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    while True:
        hb = rd.next(max_reads, min_len, max_bases)
        nb, nn = int(hb.off[-1]), int(hb.name_off[-1])
        out.append((hb.n, hb.n_short, list(hb.name_off), list(hb.off), C.string_at(hb.c.names, nn) if nn else b"",
                    C.string_at(hb.c.seqs, nb) if nb and not kw.get("names_only") else b"",
                    C.string_at(hb.c.quals, nb) if nb and not kw.get("names_only") else b""))
        if hb.n == 0:
            break
    stats = rd.parse_stats()
    rd.close()
    return out, stats


N_READS = 300


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the plain FASTQ, its BGZF forms, and the plain reader's groups per (max_reads, max_bases, min_len), computed once"""
    d = tmp_path_factory.mktemp("fq")
    text = H.fastq_text(N_READS)
    plain = str(d / "reads.fastq")
    open(plain, "wb").write(text)
    lens = sorted(len(x) for x in text.split(b"\n")[1::4])
    cut = lens[len(lens) // 3]                                              # drops about a third of the reads
    assert lens[0] < cut <= lens[-1]
    gz = {}
    for block in (37, 4096, 65280):
        gz[block] = str(d / ("reads%d.fastq.gz" % block))
        open(gz[block], "wb").write(H.bgzf_file(text, block=block, level=1 if block == 37 else 6))
    want = {}

    def ref(max_reads, max_bases, min_len):
        key = (max_reads, max_bases, min_len)
        if key not in want:
            want[key] = _groups(plain, *key)[0]
        return want[key]
    return {"text": text, "plain": plain, "gz": gz, "cut": cut, "ref": ref, "dir": d}


@pytest.mark.parametrize("stretch", [1, 3, 4096])
@pytest.mark.parametrize("block", [37, 4096, 65280])
def test_reader_equals_plain_reader(corpus, monkeypatch, block, stretch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
    cut = corpus["cut"]
    if stretch == 4096:
        params = [(mr, mb, ml) for mr in (1, 7, 1000) for mb in (0, 5000) for ml in (0, cut)]
    elif block == 37:
        # tens of thousands of stretches, each a launch sequence of its own (the cost of these two cases is their stretch count):
        # one setting each; with the cases above every value of the three parameters is met at every payload
        params = [(7, 5000, cut)] if stretch == 1 else [(1000, 0, 0)]
    else:
        params = [(1, 0, cut), (7, 5000, 0), (1000, 0, cut)]
    for mr, mb, ml in params:
        got, stats = _groups(corpus["gz"][block], mr, mb, ml, inflate_device=0, parse_device=True)
        assert got == corpus["ref"](mr, mb, ml), (block, stretch, mr, mb, ml)
        assert stats[1] == 0 and stats[2] == N_READS and stats[0] >= 1, (block, stretch, stats)
    if block == 4096:
        n_members = len(corpus["text"]) // block + 1
        _g, stats = _groups(corpus["gz"][block], 1000, 0, 0, inflate_device=0, parse_device=True)
        assert stats[0] == -(-n_members // stretch)                        # the hook does cut the stretches


def test_reader_names_only(corpus, monkeypatch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", "3")
    want = _groups(corpus["plain"], 7, 0, corpus["cut"], names_only=True)[0]
    got, stats = _groups(corpus["gz"][4096], 7, 0, corpus["cut"], names_only=True, inflate_device=0, parse_device=True)
    assert got == want and stats[1] == 0 and stats[2] == N_READS


def test_reader_falls_back_at_a_departure(corpus, monkeypatch):
    recs = corpus["text"].split(b"\n")[:-1]
    recs = [recs[i:i + 4] for i in range(0, len(recs), 4)]
    k = len(recs) // 2
    h, s, p, q = recs[k]
    m = len(s) // 3
    pieces = [b"\n".join(r) + b"\n" for r in recs]
    pieces[k] = b"\n".join([h, s[:m], s[m:], p, q[:m + 5], q[m + 5:]]) + b"\n"        # one multi-line record ...
    pieces[k + 20] = b"\n" + pieces[k + 20]                                           # ... and, later, one blank line
    text = b"".join(pieces)
    d = corpus["dir"]
    plain, gz = str(d / "multi.fastq"), str(d / "multi.fastq.gz")
    open(plain, "wb").write(text)
    open(gz, "wb").write(H.bgzf_file(text, block=4096))
    for stretch in (3, 4096):
        monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
        for mr, mb, ml in ((7, 0, 0), (1000, 5000, corpus["cut"]), (1, 0, 0)):
            want = _groups(plain, mr, mb, ml)[0]
            assert sum(g[0] + g[1] for g in want) == N_READS
            got, stats = _groups(gz, mr, mb, ml, inflate_device=0, parse_device=True)
            assert got == want, (stretch, mr, mb, ml)
            assert stats[0] >= 1 and stats[1] >= 1 and 0 < stats[2] <= k, (stretch, stats)
    # without the flag nothing is counted and the groups are the same
    got, stats = _groups(gz, 7, 0, 0, inflate_device=0)
    assert got == _groups(plain, 7, 0, 0)[0] and stats == (0, 0, 0)


def test_reader_errors(corpus, tmp_path):
    bad = bytearray(open(corpus["gz"][65280], "rb").read())
    bad[len(bad) // 2] ^= 0x55
    pb = str(tmp_path / "bad.fastq.gz")
    open(pb, "wb").write(bytes(bad))
    with pytest.raises(ValueError) as e0:
        _groups(pb, 7, 0, 0, inflate_device=0)
    with pytest.raises(ValueError) as e1:
        _groups(pb, 7, 0, 0, inflate_device=0, parse_device=True)
    assert str(e1.value) == str(e0.value) and "damaged" in str(e1.value)
    for kw in ({}, {"inflate_device": 0}):                                  # a plain-text reader has no device stretches to parse
        with pytest.raises(_lib.C3Error) as e:
            _lib.Reader(corpus["plain"], parse_device=True, **kw)
        assert e.value.code == _lib.E_STATE
    rd = _lib.Reader(corpus["gz"][65280], inflate_device=0)                 # too late after the first group
    assert rd.next(3).n == 3
    assert rd.lib.c3_reader_parse_on_device(rd.r, 1) == _lib.E_STATE
    rd.close()


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_cli_parse_gpu_equals_plain(tmp_path, capfd, monkeypatch):
    import test_gpu_inflate as G
    monkeypatch.setenv("C3_STREAM_STATS", "1")
    recs = G._recs(100)
    plain, text = G._run_cli(tmp_path / "a", recs)
    want = G._outputs(plain)
    assert set(want) >= {"c3poa.log"} | {"Splint1/" + f for f in G.FILES}
    bz = ("reads.fastq.gz", H.bgzf_file(text, block=4096))
    capfd.readouterr()
    got = G._run_cli(tmp_path / "b", recs, ["--inflate", "gpu", "--parse", "gpu"], reads=bz)[0]
    err = capfd.readouterr().err
    assert G._outputs(got) == want
    assert "parse_stretches_host=0 " in err + " " and "parse_records_device=%d" % len(recs) in err and "parse_stretches_device=1" in err
    # the fused route (no PSL), and a gzip file that is not BGZF: the note of --inflate gpu, read as before
    a = G._run_cli(tmp_path / "c", recs, psl=False)[0]
    b = G._run_cli(tmp_path / "d", recs, ["--inflate", "gpu", "--parse", "gpu"], psl=False, reads=bz)[0]
    assert G._outputs(a) == G._outputs(b)
    capfd.readouterr()
    pg = G._run_cli(tmp_path / "e", recs, ["--inflate", "gpu", "--parse", "gpu"], reads=("reads.fastq.gz", gzip.compress(text, 6)))[0]
    assert "only BGZF can be inflated on the GPU" in capfd.readouterr().err
    assert G._outputs(pg) == want
