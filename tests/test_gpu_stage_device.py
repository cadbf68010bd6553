"""The reader's device groups (c3_reader_stage_on_device): the groups of a stage_device reader against the plain
reader's groups, byte for byte (the device bytes copied back here with hipMemcpy); sets and their lifetime; departures; a
damaged member and the state checks."""
import ctypes as C

import pytest

from c3poa_amd import _lib
import test_inflate_host as H

pytestmark = pytest.mark.gpu

N_READS = 300
D2H = 2


@pytest.fixture(scope="module")
def hip():
    """the HIP runtime the library itself is linked to (device memory of another copy of it would be foreign to the library)"""
    _lib.load()
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    rt = C.CDLL(path)
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return rt


def _dev_bytes(hip, ptr, n):
    buf = C.create_string_buffer(max(n, 1))
    assert hip.hipMemcpy(buf, ptr, n, D2H) == 0
    return buf.raw[:n]


def _group(hip, hb, names_only=False):
    """(n, n_short, name_off, off, names, seqs, quals, kind) of one group; the bytes of a device group come from its device set"""
    nb, nn = int(hb.off[-1]), int(hb.name_off[-1])
    names = C.string_at(hb.c.names, nn) if nn else b""
    if hb.dev is not None:
        assert not hb.c.seqs and not hb.c.quals and hb.dev.bytes == nb and hb.dev.device == 0
        sq, ql = _dev_bytes(hip, hb.dev.d_seqs, nb), _dev_bytes(hip, hb.dev.d_quals, nb)
    else:
        sq = C.string_at(hb.c.seqs, nb) if nb else b""
        ql = C.string_at(hb.c.quals, nb) if nb else b""
    return (hb.n, hb.n_short, list(hb.name_off), list(hb.off), names, sq, ql, "dev" if hb.dev is not None else "host")


def _groups(hip, path, max_reads, max_bases, min_len, **kw):
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    while True:
        out.append(_group(hip, rd.next(max_reads, min_len, max_bases)))
        if out[-1][0] == 0:
            break
    stats = rd.stage_stats(), rd.parse_stats(), rd.reserved_bytes()
    rd.close()
    return out, stats


def _records(groups):
    """the concatenation of the groups as records, and the short count"""
    recs = []
    for n, _s, no, off, names, sq, ql, _k in groups:
        recs += [(names[no[i]:no[i + 1]], sq[off[i]:off[i + 1]], ql[off[i]:off[i + 1]]) for i in range(n)]
    return recs, sum(g[1] for g in groups)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, hip):
    d = tmp_path_factory.mktemp("stage")
    text = H.fastq_text(N_READS)
    plain = str(d / "reads.fastq")
    open(plain, "wb").write(text)
    lens = sorted(len(x) for x in text.split(b"\n")[1::4])
    cut = lens[len(lens) // 3]                                              # breaks the runs at about a third of the reads
    gz = {}
    for block in (4096, 65280):
        gz[block] = str(d / ("reads%d.fastq.gz" % block))
        open(gz[block], "wb").write(H.bgzf_file(text, block=block))
    want = {}

    def ref(max_reads, max_bases, min_len, path=plain):
        key = (max_reads, max_bases, min_len, path)
        if key not in want:
            want[key] = _groups(hip, path, max_reads, max_bases, min_len)[0]
        return want[key]
    return {"text": text, "plain": plain, "gz": gz, "cut": cut, "ref": ref, "dir": d}


STAGE = dict(inflate_device=0, parse_device=True, stage_device=True)


# ---- the reader ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretch", [1, 3, 4096])
@pytest.mark.parametrize("block", [4096, 65280])
def test_device_groups_equal_plain_groups(corpus, hip, monkeypatch, block, stretch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
    cut = corpus["cut"]
    for mr, mb, ml in ((1, 0, cut), (7, 5000, 0), (1000, 0, cut), (1000, 0, 0)):
        got, (stage, parse, reserved) = _groups(hip, corpus["gz"][block], mr, mb, ml, **STAGE)
        want = corpus["ref"](mr, mb, ml)
        assert [g[:7] for g in got] == [g[:7] for g in want], (block, stretch, mr, mb, ml)
        assert all(g[7] == "dev" for g in got[:-1]) and got[-1][0] == 0
        assert stage == (len(got) - 1, 0, 0), stage                        # every group on the device, no byte of them on the host
        assert parse[1] == 0 and parse[2] == N_READS
        # no page-locked seqs / quals block was allocated: what the reader holds on the host is one minimum block, the names
        assert reserved <= 1 << 20, reserved


def test_a_set_keeps_its_bytes_until_it_is_named_again(corpus, hip, monkeypatch):
    monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", "3")
    want = corpus["ref"](60, 0, 0)
    assert len(want) - 1 >= 5
    rd = _lib.Reader(corpus["gz"][4096], n_sets=2, **STAGE)
    held = {}
    for k, w in enumerate(want[:-1]):
        hb = rd.next(60, 0, 0, set_index=k % 2)
        assert _group(hip, hb)[:7] == w[:7]
        held[k % 2] = (hb, w)
        other = held.get((k + 1) % 2)
        if other:                                                           # the group of the set that was not named is still whole
            assert _group(hip, other[0])[:7] == other[1][:7], k
    assert rd.next(60, 0, 0, set_index=0).n == 0
    assert _group(hip, held[1][0])[:7] == held[1][1][:7]
    assert rd.stage_stats() == (len(want) - 1, 0, 0)
    rd.close()


def _departing(corpus, first):
    """the multi-line record and the blank line of tests/test_gpu_fastq.py's fallback test; first: the departure is record 0"""
    recs = corpus["text"].split(b"\n")[:-1]
    recs = [recs[i:i + 4] for i in range(0, len(recs), 4)]
    k = 0 if first else len(recs) // 2
    h, s, p, q = recs[k]
    m = len(s) // 3
    pieces = [b"\n".join(r) + b"\n" for r in recs]
    pieces[k] = b"\n".join([h, s[:m], s[m:], p, q[:m + 5], q[m + 5:]]) + b"\n"
    pieces[k + 20] = b"\n" + pieces[k + 20]
    text = b"".join(pieces)
    tag = "first" if first else "mid"
    plain, gz = str(corpus["dir"] / ("multi_%s.fastq" % tag)), str(corpus["dir"] / ("multi_%s.fastq.gz" % tag))
    open(plain, "wb").write(text)
    open(gz, "wb").write(H.bgzf_file(text, block=4096))
    return plain, gz, k


@pytest.mark.parametrize("first", [False, True], ids=["middle", "first_record"])
def test_departure(corpus, hip, monkeypatch, first):
    plain, gz, k = _departing(corpus, first)
    for stretch in (3, 4096):
        monkeypatch.setenv("C3_INFLATE_STRETCH_MEMBERS", str(stretch))
        for mr, mb, ml in ((7, 0, 0), (1000, 5000, corpus["cut"]), (1, 0, 0), (1000, 0, 0)):
            want = _records(corpus["ref"](mr, mb, ml, plain))
            assert len(want[0]) + want[1] == N_READS
            got, (stage, parse, _r) = _groups(hip, gz, mr, mb, ml, **STAGE)
            assert _records(got) == want, (stretch, mr, mb, ml)
            assert all(g[0] > 0 for g in got[:-1]) and got[-1][0] == 0     # n == 0 only at the end of the file
            kinds = [g[7] for g in got[:-1]]
            n_dev = kinds.count("dev")
            assert kinds == ["dev"] * n_dev + ["host"] * (len(kinds) - n_dev) and len(kinds) > n_dev      # device groups, then host groups
            if first:
                assert n_dev == 0
            else:
                assert n_dev >= 1 and sum(g[0] + g[1] for g in got[:n_dev]) <= k                  # they end in front of the departure
            host_bases = sum(g[3][-1] for g in got if g[7] == "host")
            assert stage == (n_dev, len(kinds) - n_dev, 2 * host_bases), stage
            assert parse[0] >= 1 and parse[1] >= 1


def test_damaged_member_and_states(corpus, hip, tmp_path):
    bad = bytearray(open(corpus["gz"][65280], "rb").read())
    bad[len(bad) // 2] ^= 0x55
    pb = str(tmp_path / "bad.fastq.gz")
    open(pb, "wb").write(bytes(bad))
    with pytest.raises(ValueError) as e0:
        _groups(hip, pb, 7, 0, 0, inflate_device=0, parse_device=True)
    rd = _lib.Reader(pb, n_sets=1, **STAGE)
    with pytest.raises(ValueError) as e1:
        for _k in range(N_READS):
            assert rd.next(7).n > 0
    assert str(e1.value) == str(e0.value) and "damaged" in str(e1.value)
    with pytest.raises(ValueError):                                         # and no group is delivered after it
        rd.next(7)
    rd.close()
    for kw in (dict(inflate_device=0), {}):                                 # no device parser in force
        with pytest.raises(_lib.C3Error) as e:
            _lib.Reader(corpus["gz"][65280], stage_device=True, **kw)
        assert e.value.code == _lib.E_STATE
    rd = _lib.Reader(corpus["gz"][65280], inflate_device=0, parse_device=True)
    assert rd.next(3).n == 3
    assert rd.lib.c3_reader_stage_on_device(rd.r, 1) == _lib.E_STATE        # too late after the first group
    rd.close()
    # names_only: no bases either way, nothing staged
    want = _lib.Reader(corpus["plain"], n_sets=1, names_only=True).next(1000)
    rd = _lib.Reader(corpus["gz"][65280], n_sets=1, names_only=True, **STAGE)
    hb = rd.next(1000)
    assert hb.n == want.n == N_READS and hb.dev is None and hb.names() == want.names() and list(hb.off) == list(want.off)
    rd.close()
