"""--bgzf on the GPU (k_bgzf): Bgzf.compress against the host statement byte for byte (the host test's inputs and > 800
blocks of FASTQ), and the CLI with -co --bgzf against a plain run on the PSL route and the fused route: decompressed
bytes, file names, member chains ending in the EOF member, independence of C3_WRITER_THREADS and of the group size,
two workers on one GPU, and the native reader on the compressed subreads."""
import gzip
import os
import struct
import zlib
from collections import Counter

import pytest

from c3poa_amd import _lib, synth
from test_bgzf_host import check_members, inputs, _fastq_text

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
SPLINT2 = "".join("ACGT"[x] for x in __import__("numpy").random.default_rng(11).integers(0, 4, len(SP)))     # nobody's splint
FILES = ["R2C2_Consensus.fasta", "R2C2_Consensus.fastq", "R2C2_Subreads.fastq"]


@pytest.fixture(scope="module")
def z():
    zz = _lib.Bgzf(0)
    yield zz
    zz.close()


@pytest.mark.parametrize("name", list(inputs()))
def test_device_equals_host(z, name):
    data = inputs()[name]
    got = z.compress(data)
    assert got == _lib.bgzf_compress_host(data)
    assert gzip.decompress(got + _lib.BGZF_EOF) == data
    check_members(data, got)


def test_device_equals_host_large(z):
    data = _fastq_text(6500, cfg="cfg2")
    assert len(data) > 50_000_000 and len(data) // 65280 > 800
    got = z.compress(data)
    assert got == _lib.bgzf_compress_host(data)
    assert zlib.decompress(got, 31) == data[:65280]             # first member
    assert gzip.decompress(got) == data
    # a second call on the same handle (buffers reused) and an unaligned slice
    sub = data[3:3 + 5 * 65280 + 999]
    assert z.compress(sub) == _lib.bgzf_compress_host(sub)


def test_device_refusals(z):
    import ctypes as C
    lib = _lib.load()
    out = C.create_string_buffer(65311)
    olen = C.c_int64(0)
    assert lib.c3_bgzf_compress(z.z, b"x" * 10, 10, out, 65310, C.byref(olen)) == -3
    assert lib.c3_bgzf_compress(None, b"x" * 10, 10, out, 65311, C.byref(olen)) == -3
    assert lib.c3_bgzf_compress(z.z, None, 10, out, 65311, C.byref(olen)) == -3
    assert lib.c3_bgzf_compress(z.z, b"", 0, None, 0, C.byref(olen)) == 0 and olen.value == 0


def _members(raw):
    """split a .gz file into members by BSIZE; every member must inflate"""
    pos, out = 0, []
    while pos < len(raw):
        assert raw[pos:pos + 4] == b"\x1f\x8b\x08\x04" and raw[pos + 12:pos + 14] == b"BC"
        size = struct.unpack("<H", raw[pos + 16:pos + 18])[0] + 1
        m = raw[pos:pos + size]
        assert len(m) == size
        zlib.decompress(m, 31)
        out.append(m)
        pos += size
    return out


def _recs(n=60):
    return list(synth.generate("cfg1", n_reads=n)) + list(synth.generate("cfg2", n_reads=n, start=10 ** 6))


def _run_cli(tmp_path, recs, extra=(), psl=True, env=None, monkeypatch=None):
    import C3POa
    out = str(tmp_path / "out")
    os.makedirs(out + "/tmp", exist_ok=True)
    fq = str(tmp_path / "reads.fastq")
    if not os.path.exists(fq):
        with open(fq, "w") as fh:
            for r in recs:
                fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))
    fa = str(tmp_path / "splint.fasta")
    open(fa, "w").write(">Splint1\n%s\n>Splint2\n%s\n" % (SP, SPLINT2))
    if psl:
        synth.write_psl(out + "/tmp/splint_to_read_alignments.psl", recs)
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    try:
        C3POa.main(C3POa.parse_args(["-r", fq, "-s", fa, "-o", out, "-g", "16"] + list(extra)))
    finally:
        if env:
            for k in env:
                monkeypatch.delenv(k, raising=False)
    return out + "/"


def _check_bgzf_dir(plain, gz):
    """every splint directory of the plain run holds exactly the .gz names in the --bgzf run, each a chain of members
    ending in the EOF member that inflates to the plain file; returns Splint1's compressed files"""
    dirs = sorted(d for d in os.listdir(plain) if d.startswith("Splint") and os.path.isdir(plain + d))
    assert "Splint1" in dirs and dirs == sorted(d for d in os.listdir(gz) if d.startswith("Splint") and os.path.isdir(gz + d))
    for d in dirs:
        files = sorted(os.listdir(plain + d))
        assert sorted(os.listdir(gz + d)) == sorted(f + ".gz" for f in files)
        for f in files:
            raw = open(gz + d + "/" + f + ".gz", "rb").read()
            ms = _members(raw)
            assert ms[-1] == _lib.BGZF_EOF and all(m != _lib.BGZF_EOF for m in ms[:-1])
            assert gzip.decompress(raw) == open(plain + d + "/" + f, "rb").read(), f
    assert sorted(os.listdir(gz + "Splint1")) == sorted(f + ".gz" for f in FILES)
    return {f: open(gz + "Splint1/" + f + ".gz", "rb").read() for f in FILES}


@pytest.mark.parametrize("psl", [True, False], ids=["psl", "fused"])
def test_cli_bgzf_equals_plain(tmp_path, psl):
    recs = _recs()
    plain = _run_cli(tmp_path / "a", recs, ["--consensus-fastq"], psl=psl)
    gz = _run_cli(tmp_path / "b", recs, ["-co", "--bgzf", "--consensus-fastq"], psl=psl)
    _check_bgzf_dir(plain, gz)
    if not psl:                                  # the fused route removed the directory of the splint nobody used
        assert not os.path.exists(gz + "Splint2") and not os.path.exists(plain + "Splint2")
    assert os.path.getsize(plain + "Splint1/R2C2_Subreads.fastq") > 500_000
    # --bgzf alone implies -co
    gz2 = _run_cli(tmp_path / "c", recs, ["--bgzf", "--consensus-fastq"], psl=psl)
    for f in FILES:
        assert open(gz2 + "Splint1/" + f + ".gz", "rb").read() == open(gz + "Splint1/" + f + ".gz", "rb").read()


def test_cli_bgzf_writer_threads_and_groups(tmp_path, monkeypatch):
    recs = list(synth.generate("cfg1", n_reads=4200))            # one group of >= 4096 reads: the writer cuts it into ranges
    plain = _run_cli(tmp_path / "p", recs, ["--consensus-fastq"])
    got = {}
    for tag, env in [("t1", {"C3_WRITER_THREADS": "1"}), ("t8", {"C3_WRITER_THREADS": "8"}),
                     ("g1", {"C3_WRITER_THREADS": "1", "C3_GPU_BATCH_READS": "1000"}),
                     ("g8", {"C3_WRITER_THREADS": "8", "C3_GPU_BATCH_READS": "1000"})]:
        got[tag] = _check_bgzf_dir(plain, _run_cli(tmp_path / tag, recs, ["-co", "--bgzf", "--consensus-fastq"], env=env,
                                                   monkeypatch=monkeypatch))
    assert got["t1"] == got["t8"]
    assert got["g1"] == got["g8"]
    # one call per group: one group ends in the only short member, five groups end in five
    def short_members(raw):
        return sum(struct.unpack("<I", m[-4:])[0] < 65280 for m in _members(raw)[:-1])
    assert short_members(got["t1"]["R2C2_Subreads.fastq"]) == 1
    assert short_members(got["g1"]["R2C2_Subreads.fastq"]) >= 4


def _records(text):
    lines = text.split(b"\n")
    step = 4 if text.startswith(b"@") else 2
    return Counter(tuple(lines[i:i + step]) for i in range(0, len(lines) - 1, step))


def test_cli_bgzf_two_workers_one_gpu(tmp_path, monkeypatch):
    recs = _recs(80)
    plain = _run_cli(tmp_path / "p", recs, ["--consensus-fastq"])
    gz = _run_cli(tmp_path / "g", recs, ["-co", "--bgzf", "--consensus-fastq", "-n", "2"],
                  env={"C3_DEVICE_MAP": "0,0", "C3_GPU_BATCH_READS": "32"}, monkeypatch=monkeypatch)
    for f in FILES:
        raw = open(gz + "Splint1/" + f + ".gz", "rb").read()
        assert _members(raw)[-1] == _lib.BGZF_EOF
        assert _records(gzip.decompress(raw)) == _records(open(plain + "Splint1/" + f, "rb").read()), f


def test_reader_on_bgzf_subreads(tmp_path):
    recs = _recs()
    plain = _run_cli(tmp_path / "p", recs)
    gz = _run_cli(tmp_path / "g", recs, ["--bgzf"])

    def read_all(path):
        rd = _lib.Reader(path, n_sets=1)
        out = []
        while True:
            hb = rd.next(100000, 0, 1 << 30)
            if hb.n == 0:
                break
            out += [hb.read(i) for i in range(hb.n)]
        rd.close()
        return out

    a = read_all(plain + "Splint1/R2C2_Subreads.fastq")
    b = read_all(gz + "Splint1/R2C2_Subreads.fastq.gz")
    assert len(a) > 100 and a == b
