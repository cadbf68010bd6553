"""c3_emit_group_bam_host, the host statement of k_bamout (--emit gpu --bam), against the writer that exists: its records,
decoded by the plain decoder of bam_out_cases, hold the names, bases and qualities of the files c3_write_group /
c3_write_consensus_fastq make of the same group, record for record.  The header, the limits, the way back through the project's
own BAM reader, and the command line's refusal.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_out_cases as BC
import emit_cases as EC
from c3poa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def groups():
    return {k: f() for k, f in BC.GROUPS.items()}


def check_against_writer(tmp, group, got, with_qv, zero):
    """the decoded streams of `got` against the writer's text of the same group; returns the decoded records per splint"""
    hb, res, cons, coff, qv, sid = group.arrays()
    want = BC.expected_records(EC.written_files(tmp, hb, res, cons, coff, qv if with_qv else None, sid, zero), with_qv)
    tots = BC.quality_sums(group)
    assert got.K == 2 and len(got.stream_off) == EC.N_SPLINTS * 2 + 1
    decoded, n = [], 0
    for s, (wc, ws) in enumerate(want):
        dc, ds = BC.decode_records(got.stream(2 * s)), BC.decode_records(got.stream(2 * s + 1))
        assert [r["name"] for r in dc] == [w[0] for w in wc] and [r["name"] for r in ds] == [w[0] for w in ws], s
        for r, (hd, letters, q) in zip(ds, ws):
            assert r["seq"] == letters and r["qual"] == q and r["tags"] == b"", hd
        for r, (hd, letters, q) in zip(dc, wc):
            assert r["seq"] == letters, hd
            assert r["qual"] == (q if q is not None else b"\xff" * r["l_seq"]), hd
            tot, L = tots[BC.read_key(hd)]
            n_p, rl, aq = BC.decode_tags(r["tags"])
            assert (n_p, rl) == (int(hd.split(b"_")[-2]), L) and rl == int(hd.split(b"_")[-3]), hd
            assert aq.tobytes() == np.float32(tot / L).tobytes(), (hd, aq, tot, L)
        decoded.append((dc, ds))
        n += len(dc) + len(ds)
    assert got.n_records == n
    return decoded


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("with_qv", [False, True])
@pytest.mark.parametrize("which", sorted(BC.GROUPS))
def test_records_equal_the_writers_text(groups, tmp_path, which, with_qv, zero):
    g = groups[which]
    hb, res, cons, coff, qv, sid = g.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, qv if with_qv else None, sid, EC.N_SPLINTS, zero)
    dec = check_against_writer(tmp_path, g, got, with_qv, zero)
    if which in ("empty", "nothing_kept"):
        assert got.n_records == 0 and int(got.stream_off[-1]) == 0
    else:
        assert got.n_records > 10 and len(dec[0][0]) > 0 and len(dec[0][1]) > 0
    if which == "main":
        assert all(len(x) > 0 for d in dec for x in d) and got.n_records > 600 and any(r["l_seq"] == 0 for r in dec[0][1])


def test_avgq_pins_as_float(groups):
    """the aq tag of the AVGQ_PINS reads is numpy.float32(tot / L) bit for bit"""
    g = groups["main"]
    hb, res, cons, coff, qv, sid = g.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, None, sid, EC.N_SPLINTS, True)
    recs = {BC.read_key(r["name"]): r for s in range(EC.N_SPLINTS) for r in BC.decode_records(got.stream(2 * s))}
    seen = 0
    for i, what in enumerate(g.what):
        if what.startswith("avgq_"):
            tot, L = (int(x) for x in what.split("_")[1:])
            assert BC.decode_tags(recs[g.names[i]]["tags"])[2].tobytes() == np.float32(tot / L).tobytes(), what
            seen += 1
    assert seen == len(EC.AVGQ_PINS)


def test_seams_meet_every_alignment(groups):
    """the seam group brings every piece length to every (source, destination) alignment of its packed bases, and every
    consensus length to every source alignment"""
    g = groups["seams"]
    hb, res, cons, coff, qv, sid = g.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, None, sid, EC.N_SPLINTS, True)
    subs = BC.decode_records(got.stream(1))
    src = [(int(hb.off[i]) + b) % 4 for i, r in enumerate(g.recs) for b, _e in r["subs"]]
    assert len(src) == len(subs)
    seen = {(r["l_seq"], a, (r["at"] + 36 + len(r["name"]) + 1) % 4) for r, a in zip(subs, src)}
    for ln in BC.SEAM_LENS:
        assert {(a, d) for l, a, d in seen if l == ln} == {(a, d) for a in range(4) for d in range(4)}, ln
    cons_src = {(int(coff[i + 1] - coff[i]), int(coff[i]) % 4) for i in range(hb.n) if g.what[i].startswith("cons")}
    assert cons_src == {(ln, a) for ln in BC.SEAM_LENS for a in range(4)}
    assert {r["l_seq"] for r in BC.decode_records(got.stream(0))} >= set(BC.SEAM_LENS) - {0}


def test_every_byte_value_and_quality_clamp(groups):
    """stated directly, beside the comparison with the writer's text: the code of each byte value and the stored qualities"""
    g = groups["bytes"]
    hb, res, cons, coff, qv, sid = g.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    first = BC.decode_records(got.stream(1))[0]                       # bytes0, piece (0, 256): the byte values in order
    want = ["N"] * 256
    for k, ch in enumerate(BC.CODES):
        want[ord(ch)] = ch
        want[ord(ch.lower())] = ch
    assert first["seq"] == "".join(want) and first["seq"].count("N") == 256 - 29      # 15 letters in both cases and '='
    assert first["qual"][:6] == bytes([0, 0, 0, 93, 93, 93])
    c0 = BC.decode_records(got.stream(0))[0]
    assert c0["seq"] == "".join(want) and c0["qual"][:6] == bytes([0, 0, 0, 93, 93, 93])


def test_limit_fills_stream_off_and_leaves_the_arena(groups):
    hb, res, cons, coff, qv, sid = groups["main"].arrays()
    full = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    need = int(full.stream_off[-1])
    arena = np.full(need + 64, 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need - 1, arena=arena)
    assert ei.value.code == _lib.E_LIMIT and "arena too small" in str(ei.value)
    assert list(ei.value.stream_off) == list(full.stream_off) and (arena == 0xA5).all()
    ok = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need, arena=arena)
    assert ok.streams() == full.streams() and (arena[need:] == 0xA5).all()
    # the packed form is smaller than the text: about 3/4 of the subread bytes
    text = _lib.emit_group_host(hb, res, cons, coff, None, sid, EC.N_SPLINTS, True)
    assert 0.70 < len(full.stream(1)) / len(text.stream(1)) < 0.95


def test_name_limits(tmp_path):
    ok = BC.named_group(b"N" * BC.MAX_NAME)
    hb, res, cons, coff, qv, sid = ok.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    dec = check_against_writer(tmp_path, ok, got, True, True)
    assert max(len(r["name"]) for d in dec for x in d for r in x) > BC.MAX_NAME + 10 and got.n_records == 6
    arena = np.full(1 << 16, 0xA5, dtype=np.uint8)
    for name, code, text in ((b"N" * (BC.MAX_NAME + 1), _lib.E_LIMIT, "more than 219 bytes"), (b"nul\0inside", _lib.E_ARG, "NUL")):
        hb, res, cons, coff, qv, sid = BC.named_group(name).arrays()
        with pytest.raises(_lib.C3Error) as ei:
            _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=len(arena), arena=arena)
        assert ei.value.code == code and text in str(ei.value) and "read 1" in str(ei.value), str(ei.value)
        assert (arena == 0xA5).all()
        sid[1] = -1                                                # decided from the names alone: a read that writes nothing is refused too
        with pytest.raises(_lib.C3Error) as ei:
            _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
        assert ei.value.code == code
    hb, res, cons, coff, qv, sid = BC.named_group(b"x").arrays()     # the limits of the text form stay
    res["sub_end"][0, 1] = 81
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    assert ei.value.code == _lib.E_ARG and "read 0: subread outside" in str(ei.value)
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, 65, True)
    assert ei.value.code == _lib.E_LIMIT and "more than 64 splints" in str(ei.value)


def test_header():
    hd = _lib.bam_out_header()
    text = b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:c3poa_amd\tPN:c3poa_amd\tVN:" + _lib.load().c3_version() + b"\n"
    assert hd == b"BAM\1" + len(text).to_bytes(4, "little") + text + b"\0\0\0\0"


def test_own_reader_takes_the_file_back(tmp_path):
    """header + subread records + EOF as BGZF members: c3_bam_parse_host delivers what c3_fastq_parse_host delivers for the
    FASTQ text of the same group"""
    g = BC.acgtn_group()
    hb, res, cons, coff, qv, sid = g.arrays()
    got = _lib.emit_group_bam_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    text = EC.written_files(tmp_path, hb, res, cons, coff, qv, sid, True)
    for s in range(EC.N_SPLINTS):
        for kind, fq in ((1, text[3 * s + 1]), (0, text[3 * s + 2])):          # subreads; consensus with QVs
            comp = _lib.bgzf_compress_host(_lib.bam_out_header() + got.stream(2 * s + kind)) + _lib.BGZF_EOF
            hd, recs = BC.parse_bam_file(comp)
            assert hd.startswith(b"@HD\tVN:1.6") and len(recs) > 10
            back = _lib.bam_parse_host(_lib.bgzf_decompress_host(comp), at_start=True, at_eof=True)
            want = _lib.fastq_parse_host(fq, at_eof=True)
            assert back.info["departed"] == 0 and back.info["n_kept"] == len(recs) == want.info["n_kept"]
            assert back.records() == want.records()


def test_output_tree_of_a_bam_run(tmp_path):
    """--bam names two .bam files per splint and nothing else, whatever --bgzf, -co and --consensus-fastq say; prepare writes
    the header member and removes stale text counterparts; finish ends each file with the EOF member; in fused mode the
    directory of a splint nobody hit goes, its files holding only their header"""
    from c3poa_amd import stream
    out = str(tmp_path) + "/"
    os.makedirs(out + "A")
    for stale in ("R2C2_Consensus.fasta", "R2C2_Subreads.fastq.gz", "R2C2_Consensus.fastq"):
        open(out + "A/" + stale, "w").write("old")
    tree = stream.OutputTree(out, ["A", "B"], bgzf=True, compress=True, qv=True, bam=True)
    assert tree.emit_paths == [out + s + "/R2C2_" + k + ".bam" for s in "AB" for k in ("Consensus", "Subreads")]
    tree.prepare({"A"})
    assert sorted(os.listdir(out + "A")) == ["R2C2_Consensus.bam", "R2C2_Subreads.bam"] and not os.path.exists(out + "B")
    head = open(out + "A/R2C2_Subreads.bam", "rb").read()
    assert BC.inflate_members(head) == _lib.bam_out_header()
    tree.finish()
    for p in tree.emit_paths[:2]:
        assert open(p, "rb").read() == head + _lib.BGZF_EOF
        assert BC.parse_bam_file(open(p, "rb").read())[1] == []
    fused = stream.OutputTree(out + "f/", ["A", "B"], finder_psl=out + "x.psl", bam=True)
    fused.prepare(set())
    assert all(os.path.getsize(p) == len(head) for p in fused.emit_paths)
    with open(fused.emit_paths[1], "ab") as fh:                   # a worker appends records to A's subreads
        fh.write(_lib.bgzf_compress_host(b"\x24\0\0\0" + b"\0" * 36))
    fused.finish(seen={"A"})
    assert sorted(os.listdir(out + "f/")) == ["A"] and os.path.exists(out + "x.psl")
    assert all(open(p, "rb").read().endswith(_lib.BGZF_EOF) for p in fused.emit_paths[:2])
    # without the flag the tree is what it was
    plain = stream.OutputTree(out, ["A"], qv=True)
    assert plain.emit_paths == [out + "A/R2C2_Consensus.fasta", out + "A/R2C2_Subreads.fastq", out + "A/R2C2_Consensus.fastq"]


def test_bam_needs_emit_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", "reads.fastq", "-s", "splint.fasta", "--bam"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--bam needs --emit gpu" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", "reads.fastq", "-s", "splint.fasta", "--bam", "--emit", "host"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--bam needs --emit gpu" in r.stderr
