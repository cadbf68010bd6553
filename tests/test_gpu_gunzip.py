"""gzip input on the GPU (k_gunzip: find, decode with markers, window chain, resolve): Bgzf.gunzip against the
host statement c3_gunzip_host and Python's zlib on the cases of tests/test_gunzip_host.py -- the bytes, the verdict and the
counters, which the shared procedure determines -- at piece sizes that put seams everywhere, and on a text of several
stretches.  The damaged files are the ones the host statement refuses on the CPU: the same decoder and procedure, so the
device is shown damage only to refuse it."""
import ctypes as C

import pytest

from c3poa_amd import _lib, synth
import test_gunzip_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    zz = _lib.Bgzf(0)
    yield zz
    zz.close()


def device_verdict(z, data, piece, env, monkeypatch):
    """(text or None, error code or 0, stats, message) of c3_gunzip at this piece size"""
    with monkeypatch.context() as m:
        m.setenv("C3_GUNZIP_PIECE", str(piece))
        for k, v in env.items():
            m.setenv(k, v)
        try:
            return z.gunzip(data), 0, _lib.gunzip_stats(), ""
        except _lib.C3Error as e:
            return None, e.code, None, str(e)


@pytest.mark.parametrize("piece", H.PIECES)
def test_valid_files_equal_the_host_statement(z, piece, monkeypatch):
    for name, data, env in H.valid_cases():
        want, code, st = H.host_verdict(data, piece, env, monkeypatch)
        assert code == 0 and want == H.reference(data), name
        got, dcode, dst, msg = device_verdict(z, data, piece, env, monkeypatch)
        assert dcode == 0 and got == want, (name, piece, dcode, msg)
        assert dst == st, (name, piece, dst, st)


def test_default_piece_and_several_stretches(z, monkeypatch):
    """the default piece size on zlib's own output (no fallback, as on the host), and stretches short enough that the text
    crosses many of them: position, window, CRC and length carried from one to the next"""
    monkeypatch.delenv("C3_GUNZIP_PIECE", raising=False)
    fq = H.fastq_text()
    for lv, mem in ((1, 8), (6, 8), (9, 8), (6, 1)):
        data = H.gz(fq, lv, mem)
        assert z.gunzip(data) == fq, (lv, mem)
        st = _lib.gunzip_stats()
        assert st["fallback_bytes"] == 0 and st["candidates"] == st["accepted"] + st["rejected"] and st["candidates"] >= 1, (lv, mem, st)
    data = H.gz(fq * 4, 6)
    monkeypatch.setenv("C3_GUNZIP_STRETCH", "40000")
    assert z.gunzip(data) == fq * 4
    st = _lib.gunzip_stats()
    assert st["stretches"] >= 8 and st["fallback_bytes"] == 0, st
    assert _lib.gunzip_host(data) == fq * 4 and _lib.gunzip_stats() == st


@pytest.mark.parametrize("piece", H.PIECES)
def test_damaged_files_are_refused_as_on_the_host(z, piece, monkeypatch):
    """every damaged file goes to the host statement first, which must give zlib's verdict; then one call on the device, which
    must give the same verdict with the same text.  No case is tried twice."""
    for name, data in H.damaged_cases() + H.truncations():
        want = H.reference(data)
        got, code, _st = H.host_verdict(data, piece, {}, monkeypatch)
        assert (code == 0 and got == want) if want is not None else code == _lib.E_DATA, (name, piece, code)
        if not data:
            continue
        dgot, dcode, _dst, msg = device_verdict(z, data, piece, {}, monkeypatch)
        assert dcode == code and dgot == got, (name, piece, dcode, msg)
        if code:
            with pytest.raises(_lib.C3Error) as e:
                _lib.gunzip_host(data, piece)
            assert msg.replace("c3_gunzip:", "c3_gunzip_host:") == str(e.value) and "is damaged (" in msg, (name, msg)
    fq = H.fastq_text()
    assert z.gunzip(H.gz(fq)) == fq                                 # the handle works afterwards


def test_device_arguments(z):
    lib = _lib.load()
    text = H.fastq_text()[:5000]
    data = H.gz(text)
    out, olen = C.create_string_buffer(len(text)), C.c_int64(-1)
    assert lib.c3_gunzip(z.z, data, len(data), out, len(text), C.byref(olen)) == 0 and out.raw == text and olen.value == len(text)
    assert lib.c3_gunzip(z.z, data, len(data), out, len(text) - 1, C.byref(olen)) == _lib.E_ARG
    assert "cap < inflated size" in lib.c3_last_error(None).decode()
    assert lib.c3_gunzip(z.z, None, len(data), out, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_gunzip(z.z, data, len(data), None, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_gunzip(z.z, data, len(data), out, len(text), None) == _lib.E_ARG
    assert lib.c3_gunzip(None, data, len(data), out, len(text), C.byref(olen)) == _lib.E_ARG
    assert lib.c3_gunzip(z.z, data, 0, out, len(text), C.byref(olen)) == 0 and olen.value == 0
    two = data + H.gz(text[:100])                                   # beyond cap only behind the first member: found on the way
    assert lib.c3_gunzip(z.z, two, len(two), out, len(text), C.byref(olen)) == _lib.E_ARG
    assert z.gunzip(H.gz(b"")) == b"" and z.gunzip(b"") == b""


# ---- the reader --------------------------------------------------------------------------------------------------------
def _read_all(path, **kw):
    """(records, inflate_wait, gunzip_stats) of the whole file in groups of 7"""
    rd = _lib.Reader(path, n_sets=1, **kw)
    out = []
    try:
        while True:
            hb = rd.next(7, 0, 1 << 30)
            if hb.n == 0:
                break
            out += [hb.read(i) for i in range(hb.n)]
        return out, rd.inflate_wait(), rd.gunzip_stats()
    finally:
        rd.close()


def test_reader_with_device_gunzip(tmp_path, monkeypatch):
    """the reader with gunzip_device delivers the groups of the plain reader, at stretch sizes that cut blocks and (three
    members, the last with a FEXTRA field) a member header, which the stream has to carry: it loads the file stretch by stretch.
    Alone, with parse_device (the text stays on the device for k_fastq) and with stage_device (the groups stay there too).
    Without the call the same reader goes through gzread as before."""
    import test_gpu_stage_device as S
    recs = [(r[0], r[1], r[2]) for r in synth.generate("cfg2", n_reads=160)]
    text = "".join("@%s\n%s\n+\n%s\n" % r for r in recs).encode()
    third = len(text) // 3
    one = H.gz(text)
    three = H.gz(text[:third]) + H.gz(b"") + H.with_header(H.gz(text[third:], 9), extra=b"\0" * 300, name=b"second")
    cut = len(H.gz(text[:third])) + len(H.gz(b"")) + 150                  # a stretch ends inside the third member's header
    p1, p3 = str(tmp_path / "one.fastq.gz"), str(tmp_path / "three.fastq.gz")
    open(p1, "wb").write(one)
    open(p3, "wb").write(three)
    want, w0, s0 = _read_all(p1)
    assert want == recs and w0 == 0.0 and s0["stretches"] == 0            # the parent's gzread path
    got, w, s = _read_all(p1, inflate_device=0)                           # a device, but no gunzip_device: still gzread
    assert got == recs and w == 0.0 and s["stretches"] == 0
    brecs = [(a.encode(), b.encode(), c.encode()) for a, b, c in recs]
    # (look: bytes loaded behind a stretch; 64 makes every stretch run out of them at least once, so that the block, trailer or
    # member header a boundary cuts is really carried and read again with more of the file)
    for path, stretch, look in ((p1, 30000, 4 << 20), (p1, 1 << 25, 4 << 20), (p3, cut, 64), (p3, 7000, 64), (p1, 30000, 64)):
        monkeypatch.setenv("C3_GUNZIP_STRETCH", str(stretch))
        monkeypatch.setenv("C3_GUNZIP_LOOK", str(look))
        n_str = 1 if stretch > len(one) else 3
        got, wait, st = _read_all(path, inflate_device=0, gunzip_device=True)
        assert got == recs, (path, stretch)
        assert wait > 0.0 and st["stretches"] >= n_str and st["pieces"] >= st["stretches"], (path, stretch, st)
        assert st["candidates"] == st["accepted"] + st["rejected"], (path, stretch, st)
        assert stretch < len(one) or st["fallback_bytes"] == 0, st       # (a stretch of a few pieces may hold no block start)
        # the device parser on the text the kernels left there
        rd = _lib.Reader(path, n_sets=1, inflate_device=0, gunzip_device=True, parse_device=True)
        got = []
        while True:
            hb = rd.next(7, 0, 1 << 30)
            if hb.n == 0:
                break
            got += [hb.read(i) for i in range(hb.n)]
        ps, gs, wait = rd.parse_stats(), rd.gunzip_stats(), rd.inflate_wait()
        rd.close()
        assert got == recs, (path, stretch)
        assert ps[0] >= n_str and ps[1] == 0 and ps[2] == len(recs) and gs == st and wait > 0.0, (path, stretch, ps, gs, st)
        # ... and the groups kept on the device
        hiprt = _hip()
        groups, (stage, ps2, _res) = S._groups(hiprt, path, 7, 1 << 30, 0, inflate_device=0, gunzip_device=True, parse_device=True, stage_device=True)
        assert S._records(groups)[0] == brecs, (path, stretch)
        assert all(g[7] == "dev" for g in groups if g[0]) and stage[0] == len(groups) - 1 and stage[1] == 0 and stage[2] == 0 and ps2 == ps, (stage, ps2)
    monkeypatch.delenv("C3_GUNZIP_STRETCH")
    monkeypatch.delenv("C3_GUNZIP_LOOK")
    # only a plain gzip file opened with a device takes the call
    plain = str(tmp_path / "a.fastq")
    open(plain, "wb").write(text)
    with pytest.raises(_lib.C3Error) as e:
        _lib.Reader(p1, gunzip_device=True)
    assert e.value.code == _lib.E_STATE and "c3_reader_gunzip_on_device" in str(e.value), str(e.value)
    with pytest.raises(_lib.C3Error) as e:
        _lib.Reader(p1, inflate_device=0, parse_device=True)           # the device parser on plain gzip needs the call
    assert e.value.code == _lib.E_STATE
    with pytest.raises(_lib.C3Error) as e:
        _lib.Reader(plain, inflate_device=0, gunzip_device=True)
    assert e.value.code == _lib.E_STATE and "not a plain gzip file" in str(e.value)


def _hip():
    """the HIP runtime the library is linked to (tests/test_gpu_stage_device.py's fixture, as a function)"""
    _lib.load()
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    rt = C.CDLL(path)
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return rt


def test_reader_refuses_a_damaged_file(tmp_path):
    """the host statement refuses the file on the CPU first; the reader then raises with the text and ends"""
    text = H.fastq_text()
    bad = bytearray(H.gz(text))
    bad[len(bad) // 2] ^= 0x55
    assert H.reference(bytes(bad)) is None
    with pytest.raises(_lib.C3Error):
        _lib.gunzip_host(bytes(bad))
    pb = str(tmp_path / "bad.fastq.gz")
    open(pb, "wb").write(bytes(bad))
    with pytest.raises(ValueError) as e:
        _read_all(pb, inflate_device=0, gunzip_device=True)
    assert "is damaged (" in str(e.value) and "member 0 at offset 0" in str(e.value), str(e.value)


# ---- the command line ---------------------------------------------------------------------------------------------------
def test_cli_gunzip_gpu_equals_plain(tmp_path, capfd):
    import gzip
    import test_gpu_inflate as G
    recs = G._recs()
    plain, text = G._run_cli(tmp_path / "a", recs)
    want = G._outputs(plain)
    assert len(want["Splint1/R2C2_Subreads.fastq"]) > 500_000
    pg = ("reads.fastq.gz", gzip.compress(text, 6))
    capfd.readouterr()
    got = G._run_cli(tmp_path / "b", recs, ["--inflate", "gpu", "--gunzip", "gpu"], reads=pg)[0]
    assert G._outputs(got) == want
    assert "only BGZF" not in capfd.readouterr().err
    got = G._run_cli(tmp_path / "c", recs, ["--inflate", "gpu", "--gunzip", "gpu", "--parse", "gpu"], reads=pg)[0]
    assert G._outputs(got) == want
    err = capfd.readouterr().err
    assert "only BGZF" not in err and "parsed on the host" not in err      # k_fastq on the text the k_gunzip kernels left on the device
    bz = ("reads.fastq.gz", G.H.bgzf_file(text, block=4096))               # --gunzip gpu changes nothing for BGZF and plain text
    assert G._outputs(G._run_cli(tmp_path / "d", recs, ["--inflate", "gpu", "--gunzip", "gpu"], reads=bz)[0]) == want
    assert G._outputs(G._run_cli(tmp_path / "e", recs, ["--inflate", "gpu", "--gunzip", "gpu"])[0]) == want


def test_cli_gunzip_gpu_needs_inflate_gpu(capsys):
    import C3POa
    with pytest.raises(SystemExit) as e:
        C3POa.parse_args(["-r", "x.fastq.gz", "-s", "s.fasta", "-o", "out", "--gunzip", "gpu"])
    assert e.value.code != 0 and "--gunzip gpu needs --inflate gpu" in capsys.readouterr().err
