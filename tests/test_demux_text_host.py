"""CPU tests of C3POa_demux.py --parse gpu's host side: the host statement c3_demux_emit_text_host (c3poa_amd/csrc/c3_dsplit.cpp)
against the Python path grouped by suffix, byte for byte; the file-name table of --split; the host path of the CLI for every new
flag (reached through an index name that holds '|', searched with c3_demux_host); the argparse rules.

The golden cases run whole and in pieces of 1, 7, 300, 301 and 4096 fresh bytes.  Cutting at EVERY byte runs on the golden
`empty_index` case in both kinds (2 KB; empty index names and an empty index) and on texts of three records made from the golden
reads (demux_text_cases.small_text: one kept record cut to 301 bases, one dropped at 300, one wrapped).  `custom_indexes` (9 KB)
and `paper` (70 KB) are not cut at every byte: every cut is three statement calls over the whole text, each searching every
kept head with the textbook search.  One flag set on `custom_indexes` takes 3 minutes as FASTA and 7 as FASTQ; `paper` is eight
times as long and the cost grows with the square of the length."""
import ctypes as C
import gzip
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from c3poa_amd import _lib, demux
from demux_emit_cases import ROOT, fnv1a, sets_of
from demux_text_cases import (IN_BGZF, KEEP_QUALS, OUT_BGZF, SPLIT, compressed, feed_pieces, golden_texts, gunzip_members, model_streams,
                              records_of, ref_strict_fastq, small_text, stream_table)

CLI = os.path.join(ROOT, "C3POa_demux.py")


def flag_sets(kind):
    return [f for f in (sum(c) for n in range(4) for c in itertools.combinations((OUT_BGZF, KEEP_QUALS, SPLIT), n)) if kind == 4 or not f & KEEP_QUALS]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    return golden_texts(tmp_path_factory.mktemp("demux_text"))


def test_statement_against_python_model_every_flag(texts, tmp_path):
    assert [t[0] for t in texts] == ["custom_indexes", "custom_indexes_fq", "empty_index", "empty_index_fq", "paper", "paper_fq"]
    for tag, kind, text, nx, tso in texts:
        sets = sets_of(nx, tso)
        S = stream_table(nx, tso)[1]
        assert S == sets.n_split_streams
        for flags in flag_sets(kind):
            want, n_reads = model_streams(text, kind, nx, tso, tmp_path, flags, tag)
            r = _lib.demux_emit_text_host(sets, text, at_eof=True, kind=kind, flags=flags)
            assert r.guards_intact and r.untouched_beyond_results, (tag, flags)
            assert r.info["departed"] == 0 and r.info["consumed"] == r.info["text_bytes"] == len(text) and r.info["kind"] == kind
            assert r.info["n_records"] == n_reads == r.hashes.size == np.unique(r.hashes).size
            assert r.info["n_streams"] == len(want) == (S if flags & SPLIT else 1) == len(r.stream_off) - 1
            assert r.info["n_kept"] == sum(len(records_of(s, flags & KEEP_QUALS)) for s in want) > 0
            assert r.streams() == (compressed(want) if flags & OUT_BGZF else want), (tag, flags)
            assert r.info["out_bytes"] == r.stream_off[-1] == sum(len(s) for s in r.streams())
            if flags & OUT_BGZF:
                assert [gunzip_members(s) for s in r.streams()] == want
        if kind == 4:
            assert b"comment" not in b"".join(_lib.demux_emit_text_host(sets, text, kind=4, flags=KEEP_QUALS).streams())
            name0 = text[1:text.index(b" ")]
            assert int(_lib.demux_emit_text_host(sets, text, kind=4).hashes[0]) == fnv1a(name0)


def test_unsplit_fasta_equals_demux_emit_host(texts):
    for tag, kind, text, nx, tso in texts:
        if kind == 2:
            sets = sets_of(nx, tso)
            r, old = _lib.demux_emit_text_host(sets, text, kind=2), _lib.demux_emit_host(text, sets)
            assert r.streams() == [old.out] and np.array_equal(r.hashes, old.hashes), tag


def test_streams_are_the_subsequences_of_the_unsplit_stream(texts):
    """independent of the model: stream s holds exactly the records of stream 0 of the unsplit call that carry its '|A_B'"""
    seen = 0
    for tag, kind, text, nx, tso in texts:
        sets = sets_of(nx, tso)
        table, S = stream_table(nx, tso)
        for keep in ((0, KEEP_QUALS) if kind == 4 else (0,)):
            whole = _lib.demux_emit_text_host(sets, text, kind=kind, flags=keep).streams()[0]
            split = _lib.demux_emit_text_host(sets, text, kind=kind, flags=keep | SPLIT).streams()
            assert sum(len(s) for s in split) == len(whole)
            recs = records_of(whole, keep)
            for name, s in table.items():
                assert split[s] == b"".join(r for r in recs if r.split(b"\n", 1)[0].endswith(b"|" + name.encode())), (tag, name)
            seen += sum(1 for s in split if s)
    assert seen > 20


@pytest.mark.parametrize("which", range(6))
def test_pieces_give_the_same_streams(texts, which):
    for tag, kind, text, nx, tso in texts[which:which + 1]:
        sets = sets_of(nx, tso)
        flags = SPLIT | (KEEP_QUALS if kind == 4 else 0)
        whole = _lib.demux_emit_text_host(sets, text, kind=kind, flags=flags)
        for fresh in (1, 7, 300, 301, 4096):
            streams, hashes, calls = feed_pieces(lambda t, e: _lib.demux_emit_text_host(sets, t, at_eof=e, kind=kind, flags=flags), text, fresh)
            assert streams == whole.streams() and np.array_equal(hashes, whole.hashes), (tag, fresh)
            assert calls >= len(text) // fresh


@pytest.mark.parametrize("source", ("three_records", "empty_index"))
@pytest.mark.parametrize("kind", (2, 4))
def test_cut_at_every_byte(kind, source, texts, tmp_path):
    """three_records: demux_text_cases.small_text, with and without SPLIT.  empty_index: the golden case whose sets hold an empty
    index and an empty index name (records '|_B' and '|A_'), as FASTA and as FASTQ, under SPLIT (and KEEP_QUALS)."""
    if source == "three_records":
        text, nx, tso = small_text(kind, tmp_path)
        flag_list = (0, SPLIT) if kind == 2 else (0, SPLIT | KEEP_QUALS)
    else:
        text, nx, tso = [t for t in texts if t[0] == ("empty_index" if kind == 2 else "empty_index_fq")][0][2:]
        flag_list = (SPLIT,) if kind == 2 else (SPLIT | KEEP_QUALS,)
    sets = sets_of(nx, tso)
    for flags in flag_list:
        emit = lambda t, e: _lib.demux_emit_text_host(sets, t, at_eof=e, kind=kind, flags=flags)      # noqa: E731
        whole = emit(text, True)
        assert whole.streams() == model_streams(text, kind, nx, tso, tmp_path, flags)[0]
        if source == "three_records":
            assert whole.info["n_records"] == 3 and whole.info["n_kept"] == 2
        else:
            heads = b"".join(r.split(b"\n", 1)[0] + b"\n" for s_ in whole.streams() for r in records_of(s_, flags & KEEP_QUALS))
            assert whole.info["n_kept"] >= 3 and b"|_" in heads and b"_\n" in heads        # empty A fields and empty B fields
        for c in range(len(text) + 1):
            head = text[:c]
            p = emit(head, False)
            assert p.info["departed"] == 0 and p.guards_intact and p.untouched_beyond_results, c
            rest = emit(text[p.info["consumed"]:], True)
            assert [a + b for a, b in zip(p.streams(), rest.streams())] == whole.streams(), c
            assert p.hashes.tolist() + rest.hashes.tolist() == whole.hashes.tolist(), c
            e = emit(head, True)                                        # the file ends here: whole records in front of the cut, or more
            assert e.guards_intact and all(w.startswith(g) or kind == 2 for g, w in zip(e.streams(), whole.streams())), c
            if kind == 2:
                assert e.info["departed"] == 0 and e.info["consumed"] == c
                if c and not flags:
                    assert e.streams() == [_lib.demux_emit_host(head, sets).out], c
            else:                                                       # the rule in Python: an incomplete record at the end of a file departs
                for r, eof in ((p, False), (e, True)):
                    recs, consumed, departed = ref_strict_fastq(head, eof)
                    assert (r.info["n_records"], r.info["consumed"], r.info["departed"]) == (len(recs), consumed, departed), (c, eof)
                    assert r.hashes.tolist() == [fnv1a(x[0]) for x in recs]


def test_limits_arguments_and_guards(texts):
    lib = _lib.load()
    tag, kind, text, nx, tso = texts[0]
    fq = texts[1][2]
    sets = sets_of(nx, tso)
    for k, t, flags in ((2, text, SPLIT), (4, fq, SPLIT | KEEP_QUALS), (4, fq, OUT_BGZF | SPLIT)):
        whole = _lib.demux_emit_text_host(sets, t, kind=k, flags=flags)
        need = int(whole.stream_off[-1]) if not flags & OUT_BGZF else sum(int(lib.c3_bgzf_bound(len(gunzip_members(s)))) for s in whole.streams() if s)
        exact = _lib.demux_emit_text_host(sets, t, kind=k, flags=flags, cap=need, max_records=whole.info["n_records"])
        assert exact.streams() == whole.streams() and exact.guards_intact
        for kw in ({"cap": need - 1, "max_records": 10 ** 4}, {"cap": 10 ** 6, "max_records": whole.info["n_records"] - 1}):
            with pytest.raises(_lib.C3Error) as e:
                _lib.demux_emit_text_host(sets, t, kind=k, flags=flags, **kw)
            assert e.value.code == _lib.E_LIMIT and e.value.untouched and e.value.guards_intact, kw
            assert e.value.info["n_records"] == whole.info["n_records"]
            if "cap" in kw and kw["cap"] == need - 1:
                assert e.value.stream_off[-1] == need and e.value.info["n_kept"] == whole.info["n_kept"]
    # KEEP_QUALS on a FASTA text, a kind that is none, BGZF members: C3_E_ARG with nothing written
    for k, t, flags in ((2, text, KEEP_QUALS), (3, text, 0), (0, text, 0), (2, text, IN_BGZF), (2, text, 16)):
        with pytest.raises(_lib.C3Error) as e:
            _lib.demux_emit_text_host(sets, t, kind=k, flags=flags)
        assert e.value.code == _lib.E_ARG and e.value.untouched and e.value.guards_intact, (k, flags)
    # more streams than C3_DEMUX_MAX_STREAMS
    big = _lib.DemuxSets(["a%d" % i for i in range(64)], ["ACGT"] * 64, ["b%d" % i for i in range(64)], ["ACGT"] * 64)
    assert big.n_split_streams == 4225
    with pytest.raises(_lib.C3Error) as e:
        _lib.demux_emit_text_host(big, text, kind=2, flags=SPLIT)
    assert e.value.code == _lib.E_LIMIT and "C3_DEMUX_MAX_STREAMS" in str(e.value) and e.value.guards_intact
    assert _lib.demux_emit_text_host(big, text, kind=2).info["n_streams"] == 1
    edge = _lib.DemuxSets(["a%d" % i for i in range(63)], ["ACGT"] * 63, ["b%d" % i for i in range(63)], ["ACGT"] * 63)
    assert _lib.demux_emit_text_host(edge, text, kind=2, flags=SPLIT).info["n_streams"] == 4096
    # the index limits and their texts are those of c3_demux_indexes
    one = _lib.DemuxSets(["A1"], ["ACGT"], ["B1", "B2"], ["AC", "GT"])
    with pytest.raises(_lib.C3Error) as e:
        _lib.demux_emit_text_host(one, text, kind=2)
    assert e.value.code == _lib.E_ARG and "at least 2 indexes" in str(e.value)
    empty = _lib.demux_emit_text_host(sets, b"", kind=4, flags=SPLIT)
    assert empty.info == {"n_records": 0, "n_kept": 0, "consumed": 0, "text_bytes": 0, "out_bytes": 0, "departed": 0, "kind": 4,
                          "n_streams": sets.n_split_streams} and not empty.stream_off.any()
    # null arguments, through the raw call
    info, st = _lib.DemuxTextInfo(), sets.struct
    out, so, hs = np.zeros(len(text) * 2, dtype=np.uint8), np.zeros(2, dtype=np.int64), np.zeros(64, dtype=np.uint64)
    args = [text, len(text), 1, 2, 0, C.byref(st), out.ctypes.data, out.size, so.ctypes.data, hs.ctypes.data, hs.size, C.byref(info)]
    assert lib.c3_demux_emit_text_host(*args) == 0 and info.n_kept > 0 and so[1] == info.out_bytes
    for k in (0, 5, 6, 8, 9, 11):
        bad = list(args)
        bad[k] = None
        assert lib.c3_demux_emit_text_host(*bad) == _lib.E_ARG, k
        assert lib.c3_demux_emit_text(None, *(bad[:3] + bad[4:])) == _lib.E_ARG, k
    assert lib.c3_demux_emit_text(None, *(args[:3] + args[4:])) == _lib.E_ARG
    assert lib.c3_demux_text_reset(None) == _lib.E_ARG and lib.c3_demux_text_timing_get(None, None) == _lib.E_ARG


def test_departures_deliver_the_records_in_front(tmp_path):
    for kind in (2, 4):
        text, nx, tso = small_text(kind, tmp_path, n=5)
        sets = sets_of(nx, tso)
        whole = _lib.demux_emit_text_host(sets, text, kind=kind, flags=SPLIT)
        starts = [i for i in range(len(text)) if text[i:i + 1] == (b">" if kind == 2 else b"@") and (i == 0 or text[i - 1:i] == b"\n")][:5]
        assert len(starts) == 5
        for at in (0, 2, 4):
            t = bytearray(text)
            t[starts[at] + 3] = 0x80
            r = _lib.demux_emit_text_host(sets, bytes(t), kind=kind, flags=SPLIT)
            assert r.info["departed"] == 1 and r.info["n_records"] == at and r.info["consumed"] == starts[at]
            front = _lib.demux_emit_text_host(sets, text[:starts[at]], kind=kind, flags=SPLIT)
            assert r.streams() == front.streams() and all(w.startswith(g) for g, w in zip(r.streams(), whole.streams()))
    text, nx, tso = small_text(2, tmp_path)
    r = _lib.demux_emit_text_host(sets_of(nx, tso), b"ACGT\n" + text, kind=2)
    assert (r.info["departed"], r.info["n_records"], r.info["consumed"], r.info["out_bytes"]) == (2, 0, 0, 0)
    fq, nx, tso = small_text(4, tmp_path)
    r = _lib.demux_emit_text_host(sets_of(nx, tso), fq.replace(b"\n+\n", b"\n-\n", 1), kind=4)
    assert (r.info["departed"], r.info["n_records"], r.info["consumed"]) == (1, 0, 0)


def test_sample_file_names():
    t = demux.sample_files(["x", "y z"], ["p", "q"])
    assert t[("x", "p")] == "x_p" and t[("y z", "")] == "y z_" and t[("", "")] == "_" and len(t) == 9
    for a, b in ((["a/b", "c"], ["p", "q"]), (["a", "c"], ["p\0", "q"]), (["x_y", "x"], ["", "y_"])):
        with pytest.raises(demux.DemuxError):
            demux.sample_files(a, b)
    with pytest.raises(demux.DemuxError) as e:
        demux.sample_files(["x_y", "x"], ["k", "y_"])             # A = x_y, B = '' against A = x, B = y_
    assert "x_y_" in str(e.value)


def run_cli(*argv):
    return subprocess.run([sys.executable, CLI] + [str(a) for a in argv], capture_output=True, text=True)


def tree(d):
    """{relative path: plain bytes} of an output directory (.gz files inflated, their names kept)"""
    out = {}
    for base, _dirs, files in os.walk(str(d)):
        for f in files:
            p = os.path.join(base, f)
            raw = open(p, "rb").read()
            out[os.path.relpath(p, str(d))] = gzip.decompress(raw) if f.endswith(".gz") else raw
    return out


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """~40 golden paper reads as FASTA, FASTQ and gzip of both; index files whose first Nextera name holds '|', which sends
    --parse gpu to the host path before any device is opened"""
    d = tmp_path_factory.mktemp("demux_cli")
    text, nx, tso = [t for t in golden_texts(d) if t[0] == "paper"][0][2:]
    recs = text.split(b">")[1:41]
    fa = b"".join(b">" + r for r in recs)
    from demux_text_cases import to_fastq
    fq = to_fastq(fa)
    files = {"fa": d / "in.fasta", "fq": d / "in.fastq", "fa_gz": d / "in.fasta.gz", "fq_gz": d / "in.fastq.gz"}
    files["fa"].write_bytes(fa)
    files["fq"].write_bytes(fq)
    files["fa_gz"].write_bytes(gzip.compress(fa))
    files["fq_gz"].write_bytes(gzip.compress(fq))
    piped = d / "nextera_piped.fasta"
    piped.write_text(open(nx).read().replace(">", ">lib|", 1))
    return {"dir": d, "files": files, "nx": str(piped), "tso": tso, "fa": fa, "fq": fq}


def host_cli(case, key, out, *flags):
    p = run_cli("-i", case["files"][key], "-o", out, "-n", case["nx"], "-t", case["tso"], "--emit", "gpu", "--parse", "gpu", "--search", "host",
                "--emit-stats", *flags)
    assert p.returncode == 0, p.stderr
    assert "falls back to the host path: an index name or sequence holds '|'" in p.stderr
    return p


def test_cli_host_path_for_each_flag(cli_case, tmp_path):
    c = cli_case
    want_fa = model_streams(c["fa"], 2, c["nx"], c["tso"], tmp_path)[0][0]
    assert want_fa.count(b"|lib|") > 0 and want_fa.count(b">") >= 30
    plain = tree(host_cli(c, "fa", tmp_path / "fa") and tmp_path / "fa")
    assert plain == {"Indexed_reads.fasta": want_fa}
    # FASTQ in (qualities dropped), gzip in of both kinds: the same file
    assert tree(host_cli(c, "fa_gz", tmp_path / "fa_gz") and tmp_path / "fa_gz") == plain
    fq_plain = tree(host_cli(c, "fq", tmp_path / "fq") and tmp_path / "fq")
    assert fq_plain == {"Indexed_reads.fasta": model_streams(c["fq"], 4, c["nx"], c["tso"], tmp_path)[0][0]}
    assert tree(host_cli(c, "fq_gz", tmp_path / "fq_gz") and tmp_path / "fq_gz") == fq_plain
    # --keep-quals
    kq = tree(host_cli(c, "fq", tmp_path / "kq", "--keep-quals") and tmp_path / "kq")
    assert kq == {"Indexed_reads.fastq": model_streams(c["fq"], 4, c["nx"], c["tso"], tmp_path, KEEP_QUALS)[0][0]}
    # --split: one file per sample that got a read, records in input order
    sp = tree(host_cli(c, "fa", tmp_path / "sp", "--split") and tmp_path / "sp")
    table, S = stream_table(c["nx"], c["tso"])
    streams = model_streams(c["fa"], 2, c["nx"], c["tso"], tmp_path, SPLIT)[0]
    assert sp == {os.path.join("samples", name + ".fasta"): streams[s] for name, s in table.items() if streams[s]} and len(sp) > 3
    assert any(k.startswith(os.path.join("samples", "lib|")) for k in sp)
    # --bgzf: the plain run's bytes behind gzip, one EOF member at the end of every file
    for flags, ref in ((("--bgzf",), plain), (("--bgzf", "--split"), sp)):
        out = tmp_path / ("z" + str(len(flags)))
        host_cli(c, "fa", out, *flags)
        assert tree(out) == {k + ".gz": v for k, v in ref.items()}
        for base, _d, files in os.walk(str(out)):
            for f in files:
                raw = open(os.path.join(base, f), "rb").read()
                assert raw.endswith(_lib.BGZF_EOF) and raw.count(_lib.BGZF_EOF) == 1 and raw[:4] == b"\x1f\x8b\x08\x04"
    # all together
    host_cli(c, "fq_gz", tmp_path / "all", "--split", "--keep-quals", "--bgzf")
    qs = model_streams(c["fq"], 4, c["nx"], c["tso"], tmp_path, SPLIT | KEEP_QUALS)[0]
    assert tree(tmp_path / "all") == {os.path.join("samples", name + ".fastq.gz"): qs[s] for name, s in table.items() if qs[s]}


def test_cli_host_path_edges(cli_case, tmp_path):
    c = cli_case
    # --keep-quals on a FASTA input: the message of C3POa_postprocessing.py --keep-quals, nothing left behind
    p = run_cli("-i", c["files"]["fa"], "-o", tmp_path / "kq", "-n", c["nx"], "-t", c["tso"], "--emit", "gpu", "--parse", "gpu", "--search", "host", "--keep-quals")
    assert p.returncode == 1 and ("--keep-quals: the records of %s have no quality line" % c["files"]["fa"]) in p.stderr
    assert not os.path.exists(tmp_path / "kq")
    # no read long enough: Indexed_reads.fasta.gz holding only the EOF member; --split gives samples/ and no file
    short = tmp_path / "short.fasta"
    short.write_bytes(b">a\nACGT\n>b\n" + b"A" * 300 + b"\n")
    args = ["-i", short, "-n", c["nx"], "-t", c["tso"], "--emit", "gpu", "--parse", "gpu", "--search", "host"]
    assert run_cli(*args, "-o", tmp_path / "e1", "--bgzf").returncode == 0
    assert open(tmp_path / "e1" / "Indexed_reads.fasta.gz", "rb").read() == _lib.BGZF_EOF
    assert run_cli(*args, "-o", tmp_path / "e2", "--split", "--bgzf").returncode == 0
    assert os.listdir(tmp_path / "e2") == ["samples"] and os.listdir(tmp_path / "e2" / "samples") == []
    # the file-name table is checked before any work, on the host path as on the device path: exit 1 with a message
    clash = tmp_path / "clash.fasta"
    clash.write_text(">x_y\nACGTACGT\n>x\nTTGGCCAA\n")
    clash_b = tmp_path / "clash_b.fasta"
    clash_b.write_text(">k\nGGGGCCCC\n>y_\nAAAATTTT\n")
    for nx, tso in ((clash, clash_b), (c["nx"].replace("nextera_piped", "slash"), c["tso"])):
        if "slash" in str(nx):
            open(nx, "w").write(">a/b\nACGTACGT\n>c\nTTGGCCAA\n")
        p = run_cli("-i", c["files"]["fa"], "-o", tmp_path / "bad", "-n", nx, "-t", tso, "--emit", "gpu", "--parse", "gpu", "--search", "host", "--split")
        assert p.returncode == 1 and "C3POa_demux: --split:" in p.stderr and not os.path.exists(tmp_path / "bad")


def test_new_flags_need_parse_gpu(cli_case, tmp_path):
    c = cli_case
    base = ["-i", c["files"]["fa"], "-o", tmp_path / "o", "-n", c["nx"], "-t", c["tso"]]
    for flags, needs in ((("--parse", "gpu"), "--parse gpu needs --emit gpu"), (("--emit", "gpu", "--split"), "--split needs --parse gpu"),
                         (("--emit", "gpu", "--keep-quals"), "--keep-quals needs --parse gpu"), (("--emit", "gpu", "--bgzf"), "--bgzf needs --parse gpu"),
                         (("--emit", "gpu", "--inflate", "gpu"), "--inflate gpu needs --parse gpu"), (("--split",), "--split needs --parse gpu")):
        p = run_cli(*base, *flags)
        assert p.returncode == 2 and needs in p.stderr and "usage:" in p.stderr, flags
    assert not os.path.exists(tmp_path / "o")
