"""--emit gpu --bam (k_bamout): c3_emit_group_bam against its host statement, byte for byte, on the hand-made groups of
bam_out_cases; the resident path (emit snapshot with C3_EMIT_BAM, with and without k_bgzf) against the host statement applied
to the fetched results; and the CLI's .bam files against the records of a plain run, read back through the plain decoder and
through the project's own reader."""
import os

import numpy as np
import pytest

import bam_out_cases as BC
import emit_cases as EC
from c3poa_amd import _lib, synth

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
SPLINT2 = "".join("ACGT"[x] for x in np.random.default_rng(11).integers(0, 4, len(SP)))


@pytest.fixture(scope="module")
def h():
    hh = _lib.Handle()
    hh.set_splints([SP, SPLINT2])
    yield hh
    hh.close()


def _same(got, want, what):
    assert list(got.stream_off) == list(want.stream_off) and got.n_records == want.n_records, what
    for x, (a, b) in enumerate(zip(got.streams(), want.streams())):
        assert a == b, "stream %d of %s differs (first at %d of %d)" % (x, what, next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), -1), len(b))


@pytest.mark.parametrize("with_qv", [False, True])
@pytest.mark.parametrize("which", sorted(BC.GROUPS))
def test_device_equals_host_statement(h, which, with_qv):
    hb, res, cons, coff, qv, sid = BC.GROUPS[which]().arrays()
    q = qv if with_qv else None
    for zero in (True, False):
        _same(h.emit_group_bam(hb, res, cons, coff, q, sid, EC.N_SPLINTS, zero), _lib.emit_group_bam_host(hb, res, cons, coff, q, sid, EC.N_SPLINTS, zero), (which, zero))
    one = np.where(sid == 1, 0, sid).astype(np.int16)             # one splint: every read in the same two streams
    want = _lib.emit_group_bam_host(hb, res, cons, coff, q, one, 1, True)
    _same(h.emit_group_bam(hb, res, cons, coff, q, one, 1, True), want, (which, "one splint"))
    if which == "main":
        t = h.emit_timing()
        assert t["n_reads"] == hb.n and t["out_bytes"] == int(want.stream_off[-1]) and t["ms_write"] > 0


def test_device_limit_and_refusals(h):
    hb, res, cons, coff, qv, sid = EC.main_group().arrays()
    full = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    need = int(full.stream_off[-1])
    arena = np.full(need + 64, 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.C3Error) as ei:
        h.emit_group_bam(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need - 1, arena=arena)
    assert ei.value.code == _lib.E_LIMIT and list(ei.value.stream_off) == list(full.stream_off) and (arena == 0xA5).all()
    got = h.emit_group_bam(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need, arena=arena)
    assert got.streams() == full.streams() and (arena[need:] == 0xA5).all()
    for name, code, text in ((b"N" * (BC.MAX_NAME + 1), _lib.E_LIMIT, "more than 219 bytes"), (b"nul\0inside", _lib.E_ARG, "NUL")):
        g = BC.named_group(name).arrays()                          # refused on the host, before any launch
        with pytest.raises(_lib.C3Error) as ei:
            h.emit_group_bam(g[0], g[1], g[2], g[3], g[4], g[5], EC.N_SPLINTS, True)
        assert ei.value.code == code and text in str(ei.value) and "read 1" in str(ei.value)
    g = BC.named_group(b"N" * BC.MAX_NAME).arrays()
    _same(h.emit_group_bam(g[0], g[1], g[2], g[3], g[4], g[5], EC.N_SPLINTS, True), _lib.emit_group_bam_host(g[0], g[1], g[2], g[3], g[4], g[5], EC.N_SPLINTS, True), "219")


def _batch(n, start):
    """n synth reads over the two splints of the handle (every third on the second, one in 17 unassigned), one read above
    TX_LONG bases and two zero-repeat reads"""
    recs, sid = [], []
    for i in range(n):
        s = 1 if i % 3 == 1 else 0
        recs += list(synth.generate("cfg1" if i % 2 else "cfg2", n_reads=1, start=start + i + (10 ** 6 if s else 0), splint=SPLINT2 if s else SP))
        sid.append(-1 if i % 17 == 5 else s)
    big = next(iter(synth.generate("cfg2", n_reads=1, start=start + 777)))
    long_read = ("long", big[1] * 8, big[2] * 8) + big[3:]        # one molecule, eight times the passes
    assert len(long_read[1]) > BC.TX_LONG
    recs.append(long_read)
    recs += [("zero%d" % k,) + synth.make_zero_read(np.random.default_rng([5, start, k]), SP, 900, 200, 700) for k in range(2)]
    sid = np.array(sid + [0] * 3, dtype=np.int16)
    st = "".join("?" if s < 0 else r[3] for s, r in zip(sid, recs))
    hb = _lib.HostBatch.from_lists([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
    return hb, sid, st


@pytest.fixture(scope="module")
def resident(h):
    """one batch of 43 reads run with QVs; its BAM snapshot fetched plain (after a refused second snapshot and a fetch with a
    small arena), then once more through k_bgzf; then run without QVs and fetched plain"""
    out = {}
    hb, sid, st = _batch(40, 0)
    h.upload_host(hb, st, np.maximum(sid, 0))
    h.run(qv=True)
    shape = h.results_snapshot()
    ns = h.emit_snapshot(hb, True, False, True, bam=True)
    assert ns == 4
    with pytest.raises(_lib.C3Error) as ei:
        h.emit_snapshot(hb, True, False, True, bam=True)
    out["second_snapshot_code"] = ei.value.code
    rb, eb = _lib.ResultBuffers(), _lib.EmitBuffers()
    res, buf, coff, qv = h.results_fetch_qv(rb, shape)
    so = np.zeros(ns + 1, dtype=np.int64)
    out["small_cap_code"] = h.lib.c3_batch_emit_fetch(h.h, eb.ptr, 16, so.ctypes.data)
    out["small_cap_need"] = int(so[ns])
    eb, so = h.emit_fetch(eb, ns)                                  # the snapshot was kept
    out.update(hb=hb, sid=sid, res=res.copy(), cons=buf.copy(), coff=coff.copy(), qv=qv.copy(), so=so.copy(), arena=eb.arr[:int(so[-1])].copy())
    ns = h.emit_snapshot(hb, True, True, True, bam=True)           # the batch is still resident: the same streams as BGZF members
    eb, so = h.emit_fetch(eb, ns)
    out.update(so_z=so.copy(), arena_z=eb.arr[:int(so[-1])].copy())
    h.upload_host(hb, st, np.maximum(sid, 0))
    h.run()
    shape = h.results_snapshot()
    ns = h.emit_snapshot(hb, True, False, False, bam=True)
    res, buf, coff = h.results_fetch(rb, shape)
    eb, so = h.emit_fetch(eb, ns)
    out.update(res_n=res.copy(), cons_n=buf.copy(), coff_n=coff.copy(), so_n=so.copy(), arena_n=eb.arr[:int(so[-1])].copy())
    eb.close()
    return out


def test_resident_equals_host_statement(h, resident):
    r = resident
    assert r["second_snapshot_code"] == _lib.E_STATE
    want = _lib.emit_group_bam_host(r["hb"], r["res"], r["cons"], r["coff"], r["qv"], r["sid"], 2, True)
    assert r["small_cap_code"] == _lib.E_LIMIT and r["small_cap_need"] == int(want.stream_off[-1])
    assert list(r["so"]) == list(want.stream_off)
    assert r["arena"].tobytes() == want.arena[:int(want.stream_off[-1])].tobytes()
    assert (np.diff(want.stream_off) > 2000).all()                # both splints, both kinds
    cons0 = BC.decode_records(want.stream(0))
    assert len(cons0) > 15 and all(c["qual"][:1] != b"\xff" for c in cons0)
    assert any(s["l_seq"] > 500 and s["name"].startswith(b"long_") for s in BC.decode_records(want.stream(1)))      # the shared read writes
    with pytest.raises(_lib.C3Error) as ei:                       # nothing is frozen any more
        h.emit_fetch(_lib.EmitBuffers(), 4)
    assert ei.value.code == _lib.E_STATE


def test_resident_bgzf_and_without_qv(resident):
    r = resident
    want = _lib.emit_group_bam_host(r["hb"], r["res"], r["cons"], r["coff"], r["qv"], r["sid"], 2, True)
    for x in range(4):
        comp = r["arena_z"][int(r["so_z"][x]):int(r["so_z"][x + 1])].tobytes()
        assert _lib.bgzf_decompress_host(comp) == want.stream(x) and BC.inflate_members(comp) == want.stream(x), x
    assert len(want.stream(1)) > 65280                            # more than one member: records straddle them
    plain = _lib.emit_group_bam_host(r["hb"], r["res_n"], r["cons_n"], r["coff_n"], None, r["sid"], 2, True)
    assert list(r["so_n"]) == list(plain.stream_off) and r["arena_n"].tobytes() == plain.arena[:int(plain.stream_off[-1])].tobytes()
    assert all(c["qual"] == b"\xff" * c["l_seq"] for c in BC.decode_records(plain.stream(0)))


def _run_cli(tmp_path, recs, extra=(), psl=True):
    import C3POa
    out = str(tmp_path / "out")
    os.makedirs(out + "/tmp", exist_ok=True)
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "w") as fh:
        for r in recs:
            fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))
    fa = str(tmp_path / "splint.fasta")
    open(fa, "w").write(">Splint1\n%s\n>Splint2\n%s\n" % (SP, SPLINT2))
    if psl:
        with open(out + "/tmp/splint_to_read_alignments.psl", "w") as fh:     # synth.write_psl's rows, each read on its own splint
            for name, seq, _q, strand, _t in recs:
                fh.write("\t".join(["280", "4", "0", "0", "0", "0", "0", "0", strand, name, str(len(seq)), "0", "284",
                                    "Splint2" if name.startswith("s2_") else "Splint1", "284", "0", "284", "1", "284,", "0,", "0,"]) + "\n")
    C3POa.main(C3POa.parse_args(["-r", fq, "-s", fa, "-o", out, "-g", "16"] + list(extra)))
    return out + "/"


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _s, fs in os.walk(root) for f in fs if f.startswith("R2C2_"))


@pytest.fixture(scope="module")
def cli_recs():
    """60 reads, interleaved: two of three on Splint1, every third on Splint2 (its names begin with s2_), two zero-repeat reads"""
    a = list(synth.generate("cfg1", n_reads=20)) + list(synth.generate("cfg2", n_reads=20, start=10 ** 6))
    b = [("s2_" + r[0],) + r[1:] for r in synth.generate("cfg2", n_reads=20, start=2 * 10 ** 6, splint=SPLINT2)]
    recs = []
    for k in range(20):
        recs += a[2 * k:2 * k + 2] + b[k:k + 1]
    return recs + [("zero%d" % k,) + synth.make_zero_read(np.random.default_rng([9, k]), SP, 900, 200, 700) for k in range(2)]


@pytest.mark.parametrize("extra", [[], ["--consensus-fastq"]], ids=["plain", "fastq"])
def test_cli_bam_holds_the_records_of_the_plain_run(tmp_path, monkeypatch, cli_recs, extra):
    monkeypatch.setenv("C3_GPU_BATCH_READS", "32")               # two batches
    qv = bool(extra)
    text = _run_cli(tmp_path / "text", cli_recs, extra)
    bam = _run_cli(tmp_path / "bam", cli_recs, extra + ["--emit", "gpu", "--bam", "--bgzf"])
    assert _files(bam) == sorted("%s/R2C2_%s.bam" % (sp, k) for sp in ("Splint1", "Splint2") for k in ("Consensus", "Subreads"))
    for sp in ("Splint1", "Splint2"):
        fa = BC.parse_fasta(open(text + sp + "/R2C2_Consensus.fasta", "rb").read())
        subs = BC.parse_sub_fastq(open(text + sp + "/R2C2_Subreads.fastq", "rb").read())
        hd, recs = BC.parse_bam_file(open(bam + sp + "/R2C2_Subreads.bam", "rb").read())
        assert b"@PG\tID:c3poa_amd" in hd and len(recs) > 50
        assert [(r["name"], r["seq"], r["qual"], r["tags"]) for r in recs] == [(n, BC.mapped(s), BC.clamped(q), b"") for n, s, q in subs]
        _hd, recs = BC.parse_bam_file(open(bam + sp + "/R2C2_Consensus.bam", "rb").read())
        assert [(r["name"], r["seq"]) for r in recs] == [(n, BC.mapped(s)) for n, s in fa] and len(recs) >= 15
        if qv:
            fq = BC.parse_cons_fastq(open(text + sp + "/R2C2_Consensus.fastq", "rb").read())
            assert [r["qual"] for r in recs] == [BC.clamped(q) for _n, _s, q in fq]
        else:
            assert all(r["qual"] == b"\xff" * r["l_seq"] for r in recs)
        for r in recs:
            n_p, rl, aq = BC.decode_tags(r["tags"])
            f = r["name"].split(b"_")
            assert (n_p, rl) == (int(f[-2]), int(f[-3])) and abs(float(aq) - float(f[-4])) <= 0.005 + 1e-4, r["name"]
        # the project's own reader: the same records from the .bam as from the plain run's .fastq
        assert BC.reader_records(bam + sp + "/R2C2_Subreads.bam") == BC.reader_records(text + sp + "/R2C2_Subreads.fastq")


def test_cli_bam_fused_drops_the_unused_splint(tmp_path, monkeypatch, cli_recs):
    """no PSL: the splints are found on the GPU, every .bam is prepared with its header, and the splint nobody hit goes"""
    monkeypatch.setenv("C3_GPU_BATCH_READS", "32")
    recs = [r for r in cli_recs if not r[0].startswith("s2_")]
    out = _run_cli(tmp_path, recs, ["--emit", "gpu", "--bam"], psl=False)
    assert _files(out) == ["Splint1/R2C2_Consensus.bam", "Splint1/R2C2_Subreads.bam"] and not os.path.exists(out + "Splint2")
    _hd, cons = BC.parse_bam_file(open(out + "Splint1/R2C2_Consensus.bam", "rb").read())
    assert len(cons) >= 30
