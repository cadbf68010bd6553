"""--inflate gpu (k_inflate): Bgzf.decompress against Python's zlib on the corpora of tests/test_inflate_host.py (valid,
hand-made, damaged, badly framed) and on > 50 MB of FASTQ, the native reader with a device inflater against the plain
file, and the CLI with --inflate gpu against the run on the plain FASTQ.  The damaged corpus is the one the host statement
refuses on the CPU (test_inflate_host.py): the same decoder, so the device is shown damage only to refuse it."""
import gzip
import os
import zlib

import pytest

from c3poa_amd import _lib, synth
import test_inflate_host as H

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
SPLINT2 = "".join("ACGT"[x] for x in __import__("numpy").random.default_rng(11).integers(0, 4, len(SP)))     # nobody's splint
FILES = ["R2C2_Consensus.fasta", "R2C2_Consensus.fastq", "R2C2_Subreads.fastq"]


@pytest.fixture(scope="module")
def z():
    zz = _lib.Bgzf(0)
    yield zz
    zz.close()


def test_valid_corpus(z):
    for name, data, text in H.valid_corpus():
        assert z.decompress(data) == text, name


def test_handmade_dynamic_headers(z):
    H.check_verdicts(z.decompress, [(n, H.handmade_member(p)) for n, p in H.dynamic_header_members()])
    assert z.decompress(H.bgzf_file(b"still works")) == b"still works"


def test_large(z):
    text = H.fastq_text(6500)
    assert len(text) > 50_000_000
    assert z.decompress(H.bgzf_file(text)) == text                  # full members: one chunk
    data = H.bgzf_file(text, block=6000)
    assert _lib.bgzf_scan(data)[0] > 2 * 4096                       # more members than two chunks
    assert z.decompress(data) == text
    sub = text[3:3 + 5 * 65280 + 999]                               # a second call on the same handle
    assert z.decompress(H.bgzf_file(sub, level=9)) == sub
    assert z.decompress(H.bgzf_file(text[:3_000_000], level=0)) == text[:3_000_000]         # all members stored
    own = z.compress(text)                                          # k_bgzf's own output
    assert z.decompress(own) == text
    assert z.decompress(own + _lib.BGZF_EOF) == text


def test_damaged_and_framing(z):
    cases = H.damaged_corpus()
    assert len(cases) == 5 * 203
    # the host statement refuses them on the CPU first (the same check as test_inflate_host.py) ...
    H.check_verdicts(_lib.bgzf_decompress_host, cases)
    # ... then the device, one call per case and one call with the first damaged member in the middle of good ones
    H.check_verdicts(z.decompress, cases)
    good = H.bgzf_members(H.fastq_text(), block=4096)
    bad = next(m for _n, m in cases if H.ref_member(m) is None)
    with pytest.raises(_lib.C3Error) as e:
        z.decompress(b"".join(good[:7]) + bad + b"".join(good[7:]) + H.EOF_MEMBER)
    assert e.value.code == _lib.E_DATA and "member 7 " in str(e.value)
    for name, data in H.framing_cases():
        with pytest.raises(_lib.C3Error) as e:
            z.decompress(data)
        assert e.value.code == _lib.E_DATA, name
    text = H.fastq_text()
    assert z.decompress(H.bgzf_file(text)) == text                  # the handle works afterwards


def test_device_arguments(z):
    import ctypes as C
    lib = _lib.load()
    text = H.fastq_text(8)
    data = H.bgzf_file(text)
    out, olen = C.create_string_buffer(len(text)), C.c_int64(-1)
    assert lib.c3_bgzf_decompress(z.z, data, len(data), out, len(text), C.byref(olen)) == 0 and out.raw == text
    assert lib.c3_bgzf_decompress(z.z, data, len(data), out, len(text) - 1, C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress(z.z, None, len(data), out, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress(z.z, data, len(data), None, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress(z.z, data, len(data), out, len(text), None) == _lib.E_ARG
    assert lib.c3_bgzf_decompress(None, data, len(data), out, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_bgzf_decompress(z.z, data, 0, out, len(text), C.byref(olen)) == 0 and olen.value == 0


# ---- the reader --------------------------------------------------------------------------------------------------------
def _read_all(path, **kw):
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    while True:
        hb = rd.next(7, 0, 1 << 30)
        if hb.n == 0:
            break
        out += [hb.read(i) for i in range(hb.n)]
    wait = rd.inflate_wait()
    rd.close()
    return out, wait


def test_reader_with_device_inflater(tmp_path):
    recs = [(r[0], r[1], r[2]) for r in synth.generate("cfg2", n_reads=160)]
    text = "".join("@%s\n%s\n+\n%s\n" % r for r in recs).encode()
    plain = str(tmp_path / "a.fastq")
    open(plain, "wb").write(text)
    want, w0 = _read_all(plain)
    assert want == recs and w0 == 0.0
    for block, extra in ((65280, False), (301, False), (4096, True)):
        pz = str(tmp_path / ("b%d.fastq.gz" % block))
        open(pz, "wb").write(H.bgzf_file(text, block=block, extra_first=extra))
        assert len(text) // block + 1 > 4096 or block != 301        # the small blocks span several device stretches
        got, wait = _read_all(pz, inflate_device=0)
        assert got == recs, block
        assert (wait > 0.0) == (not extra)        # (a foreign subfield in front: c3_reader_open takes the file for plain gzip, as ever)
        assert _read_all(pz)[0] == recs                             # (and the zlib threads, as before)
    bad = bytearray(open(str(tmp_path / "b65280.fastq.gz"), "rb").read())
    bad[len(bad) // 2] ^= 0x55
    pb = str(tmp_path / "bad.fastq.gz")
    open(pb, "wb").write(bytes(bad))
    with pytest.raises(ValueError):
        _read_all(pb)
    with pytest.raises(ValueError) as e:
        _read_all(pb, inflate_device=0)
    assert "damaged" in str(e.value)
    pg = str(tmp_path / "plain.fastq.gz")                           # plain gzip and plain text: read as without a device
    with gzip.open(pg, "wb") as fh:
        fh.write(text)
    assert _read_all(pg, inflate_device=0)[0] == recs
    assert _read_all(plain, inflate_device=0)[0] == recs
    with pytest.raises(OSError):
        _lib.Reader(str(tmp_path / "missing.fastq.gz"), inflate_device=0)


# ---- the command line ---------------------------------------------------------------------------------------------------
def _recs(n=60):
    return list(synth.generate("cfg1", n_reads=n)) + list(synth.generate("cfg2", n_reads=n, start=10 ** 6))


def _run_cli(tmp_path, recs, extra=(), psl=True, reads=None, capsys=None):
    """one run; reads: (file name, bytes) of the input when it is not the plain FASTQ of recs"""
    import C3POa
    out = str(tmp_path / "out")
    os.makedirs(out + "/tmp", exist_ok=True)
    text = "".join("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]) for r in recs).encode()
    name, data = reads if reads else ("reads.fastq", text)
    fq = str(tmp_path / name)
    open(fq, "wb").write(data)
    fa = str(tmp_path / "splint.fasta")
    open(fa, "w").write(">Splint1\n%s\n>Splint2\n%s\n" % (SP, SPLINT2))
    if psl:
        synth.write_psl(out + "/tmp/splint_to_read_alignments.psl", recs)
    C3POa.main(C3POa.parse_args(["-r", fq, "-s", fa, "-o", out, "-g", "16", "--consensus-fastq"] + list(extra)))
    return out + "/", text


def _outputs(out, gz=False):
    got = {"c3poa.log": open(out + "c3poa.log", "rb").read()}
    for d in sorted(x for x in os.listdir(out) if x.startswith("Splint") and os.path.isdir(out + x)):
        for f in sorted(os.listdir(out + d)):
            raw = open(out + d + "/" + f, "rb").read()
            got[d + "/" + (f[:-3] if gz else f)] = gzip.decompress(raw) if gz else raw
    return got


@pytest.mark.parametrize("psl", [True, False], ids=["psl", "fused"])
def test_cli_inflate_gpu_equals_plain(tmp_path, psl, capfd):
    recs = _recs()
    plain, text = _run_cli(tmp_path / "a", recs, psl=psl)
    want = _outputs(plain)
    assert set(want) >= {"Splint1/" + f for f in FILES} and len(want["Splint1/R2C2_Subreads.fastq"]) > 500_000
    bz = ("reads.fastq.gz", H.bgzf_file(text, block=4096))
    capfd.readouterr()
    got = _run_cli(tmp_path / "b", recs, ["--inflate", "gpu"], psl=psl, reads=bz)[0]
    assert _outputs(got) == want
    assert "only BGZF" not in capfd.readouterr().err
    assert _outputs(_run_cli(tmp_path / "c", recs, ["--inflate", "host"], psl=psl, reads=bz)[0]) == want
    # together with --bgzf: the outputs inflate to the same text
    both = _run_cli(tmp_path / "d", recs, ["--inflate", "gpu", "--bgzf"], psl=psl, reads=bz)[0]
    assert _outputs(both, gz=True) == want
    if psl:
        # the program reading its own output: the subreads of the --bgzf run as the input of a run on the fused route
        own = open(both + "Splint1/R2C2_Subreads.fastq.gz", "rb").read()
        assert gzip.decompress(own) == want["Splint1/R2C2_Subreads.fastq"]
        subs = []
        lines = want["Splint1/R2C2_Subreads.fastq"].decode().split("\n")
        for i in range(0, len(lines) - 1, 4):
            subs.append((lines[i][1:], lines[i + 1], lines[i + 3]))
        a = _run_cli(tmp_path / "e", subs, psl=False)[0]
        b = _run_cli(tmp_path / "f", subs, ["--inflate", "gpu"], psl=False, reads=("subs.fastq.gz", own))[0]
        assert _outputs(a) == _outputs(b)
    # a plain gzip input: read as before, with a note
    capfd.readouterr()
    pg = _run_cli(tmp_path / "g", recs, ["--inflate", "gpu"], psl=psl, reads=("reads.fastq.gz", gzip.compress(text, 6)))[0]
    assert "only BGZF can be inflated on the GPU" in capfd.readouterr().err
    assert _outputs(pg) == want
