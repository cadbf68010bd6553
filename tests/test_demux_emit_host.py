"""CPU tests of C3POa_demux.py --emit gpu's host side: the host statements c3_fasta_parse_host and c3_demux_emit_host
(c3poa_amd/csrc/c3_fasta.cpp) against demux.read_fasta and the Python host path, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from c3poa_amd import _lib, demux
from demux_emit_cases import (STRIP, case_files, corpus, dedup, feed_chunks, fnv1a, golden_cases, host_path_bytes, ref_parse,
                              sets_of)


def read_fasta_of(text, d, tag="t"):
    p = d / (tag + ".fa")
    p.write_bytes(text)
    return demux.read_fasta(str(p))


def as_dict(records):
    """the dict read_fasta builds from these records: first position, last sequence"""
    d = {}
    for name, seq in records:
        d[name.decode("ascii")] = seq.decode("ascii")
    return d


def test_strip_set_is_rstrip():
    assert bytes(c for c in range(128) if ("x" + chr(c)).rstrip() == "x") == STRIP


def test_parser_semantics_against_read_fasta(tmp_path):
    names = [n for n, _t in corpus()]
    for want in ("semantics", "wrapped", "crlf", "lone_cr", "strip_at_ends", "strip_inside", "empty_name", "empty_sequence",
                 "no_final_newline", "empty"):
        assert want in names
    for name, text in corpus():
        p = _lib.fasta_parse_host(text, at_eof=True)
        assert p.guards_intact and p.untouched_beyond_results, name
        assert p.info["departed"] == 0 and p.info["consumed"] == len(text), name
        assert list(as_dict(p.records()).items()) == list(read_fasta_of(text, tmp_path, name).items()), name
        assert p.records() == ref_parse(text, True)[0], name
        assert p.hashes.tolist() == [fnv1a(n) for n, _s in p.records()], name
        assert p.info["name_bytes"] == len(p.names) and p.info["base_bytes"] == len(p.seqs), name
    sem = dict(corpus())["semantics"]
    assert list(as_dict(_lib.fasta_parse_host(sem).records()).items()) == [("r 1", "CCCAA"), ("r\t2", "GG"), ("x", ""), ("", " A"), ("empty", "")]


def test_cut_at_every_byte(tmp_path):
    for name, text in corpus():
        full = _lib.fasta_parse_host(text, at_eof=True).records()
        for c in range(len(text) + 1):
            head = text[:c]
            e = _lib.fasta_parse_host(head, at_eof=True)
            assert e.info["departed"] == 0 and e.info["consumed"] == c, (name, c)
            assert list(as_dict(e.records()).items()) == list(read_fasta_of(head, tmp_path).items()), (name, c)
            p = _lib.fasta_parse_host(head, at_eof=False)
            want, consumed, departed = ref_parse(head, False)
            assert (p.records(), p.info["consumed"], p.info["departed"]) == (want, consumed, departed), (name, c)
            assert p.guards_intact and p.untouched_beyond_results, (name, c)
            rest = _lib.fasta_parse_host(text[p.info["consumed"]:], at_eof=True)
            assert p.records() + rest.records() == full, (name, c)
            assert p.hashes.tolist() + rest.hashes.tolist() == [fnv1a(n) for n, _s in full], (name, c)


def test_departures_first_middle_last():
    recs = [b">r%d\nACGT\nTT\n" % k for k in range(5)]
    for at in (0, 2, 4):
        for inside in (1, 4, 9):                                      # in the header, in the first and in the second sequence line
            t = bytearray(b"".join(recs))
            t[sum(len(r) for r in recs[:at]) + inside] = 0x80
            t = bytes(t)
            for at_eof in (False, True):
                p = _lib.fasta_parse_host(t, at_eof=at_eof)
                assert p.info["departed"] == 1 and p.info["n_records"] == at, (at, inside, at_eof)
                assert p.info["consumed"] == sum(len(r) for r in recs[:at])
                assert (p.records(), p.info["consumed"], 1) == ref_parse(t, at_eof)
    # a sequence line in front of the first header of the text: nothing is delivered, whatever follows
    for t in (b"ACGT\n>r\nACGT\n", b"\n \nAC\n>r\nAC\n", b"AC", b" >r\nAC\n", b"AC\n>r\n\x80\n", b"\x80\n>r\nAC\n"):
        for at_eof in (False, True):
            p = _lib.fasta_parse_host(t, at_eof=at_eof)
            assert (p.info["departed"], p.info["n_records"], p.info["consumed"]) == (2, 0, 0), (t, at_eof)
            assert ([], 0, 2) == ref_parse(t, at_eof)
    # ... as a later chunk of a file would look if it did not start at a header line (the middle and the end of a file reach the
    # rule only as texts that start at a header, so kind 2 there is kind 2 of the text handed over)
    assert _lib.fasta_parse_host(b">a\nAC\n>b\n\x80GT\n>c\nAC\n").info == {"n_records": 1, "consumed": 6, "name_bytes": 1, "base_bytes": 2, "departed": 1}


def test_parse_limits_and_arguments():
    lib = _lib.load()
    text = b">ab\nACGT\n>c\nGG\n"
    ok = _lib.fasta_parse_host(text, caps=(3, 6, 2))
    assert ok.records() == [(b"ab", b"ACGT"), (b"c", b"GG")] and ok.guards_intact
    for caps in ((2, 6, 2), (3, 5, 2), (3, 6, 1)):
        with pytest.raises(_lib.C3Error) as e:
            _lib.fasta_parse_host(text, caps=caps)
        assert e.value.code == _lib.E_LIMIT and e.value.untouched and e.value.guards_intact
        assert e.value.info == {"n_records": 2, "consumed": len(text), "name_bytes": 3, "base_bytes": 6, "departed": 0}
        assert "capacity too small" in str(e.value)
    info = _lib.FastaInfo()
    buf = np.zeros(64, dtype=np.uint8)
    o = np.zeros(8, dtype=np.int64)
    args = [text, len(text), 1, buf.ctypes.data, 64, o.ctypes.data, buf.ctypes.data, 64, o.ctypes.data, o.ctypes.data, 4, C.byref(info)]
    assert lib.c3_fasta_parse_host(*args) == 0 and info.n_records == 2
    for k in (0, 3, 5, 6, 8, 9, 11):
        bad = list(args)
        bad[k] = None
        assert lib.c3_fasta_parse_host(*bad) == _lib.E_ARG, k
        assert lib.c3_fasta_parse(None, *bad) == _lib.E_ARG, k
    for k, v in ((1, -1), (4, -1), (7, -1), (10, -1)):
        bad = list(args)
        bad[k] = v
        assert lib.c3_fasta_parse_host(*bad) == _lib.E_ARG, k
    assert lib.c3_fasta_parse(None, *args) == _lib.E_ARG
    big = list(args)
    big[1] = _lib.FASTA_MAX_TEXT + 1
    assert lib.c3_fasta_parse_host(*big) == _lib.E_LIMIT and b"C3_FASTA_MAX_TEXT" in lib.c3_last_error(None)
    empty = list(args)
    empty[0], empty[1] = None, 0
    assert lib.c3_fasta_parse_host(*empty) == 0 and info.n_records == 0 and info.consumed == 0


@pytest.fixture(scope="module")
def golden():
    return {c["name"]: c for c in golden_cases()}


def plain_case(case, nx, tso):
    """no high byte, no repeated header, no '|' in an index name: what lets a case through the device path"""
    text = case["input"].encode()
    names = [n for n, _s in ref_parse(text, True)[0]]
    idx = demux.load_indexes(nx)[0] + demux.load_indexes(tso)[0]
    return max(text, default=0) < 0x80 and len(set(names)) == len(names) and not any("|" in n for n in idx)


def test_emit_statement_against_python_host_path(golden, tmp_path):
    assert set(golden) >= {"paper", "custom_indexes", "empty_index"}
    for name in ("custom_indexes", "empty_index"):
        case = golden[name]
        inp, nx, tso = case_files(case, tmp_path)
        assert plain_case(case, nx, tso), name
        text = open(inp, "rb").read()
        r = _lib.demux_emit_host(text, sets_of(nx, tso))
        assert r.info["departed"] == 0 and r.info["consumed"] == len(text) and r.guards_intact and r.untouched_beyond_results
        assert np.unique(r.hashes).size == r.hashes.size == r.info["n_records"]
        assert r.out == host_path_bytes(text, nx, tso, tmp_path, name) == case["output"].encode(), name
        assert r.out.count(b"\n") == 2 * r.info["n_kept"] and r.info["out_bytes"] == len(r.out)
    case = golden["paper"]
    inp, nx, tso = case_files(case, tmp_path)
    text = open(inp, "rb").read()
    r = _lib.demux_emit_host(text, sets_of(nx, tso))
    assert r.info["departed"] == 0 and np.unique(r.hashes).size < r.hashes.size       # repeated headers: the CLI falls back
    clean = dedup(text)
    assert clean != text and len(clean) > len(text) // 2
    r = _lib.demux_emit_host(clean, sets_of(nx, tso))
    assert np.unique(r.hashes).size == r.hashes.size == r.info["n_records"] > 0
    assert r.out == host_path_bytes(clean, nx, tso, tmp_path, "paper_dedup")
    assert r.info["n_kept"] > 0 and b"|_" in r.out and b"_\n" in r.out            # calls and no-calls


def test_emit_in_chunks_gives_the_same_bytes(golden, tmp_path):
    for name in ("custom_indexes", "empty_index", "paper"):
        inp, nx, tso = case_files(golden[name], tmp_path)
        text = open(inp, "rb").read()
        if name == "paper":
            text = dedup(text)
        sets = sets_of(nx, tso)
        whole = _lib.demux_emit_host(text, sets)
        for fresh in (1, 7, 300, 301, 4096):
            out, hashes, calls = feed_chunks(lambda t, e: _lib.demux_emit_host(t, sets, at_eof=e), text, fresh)
            assert out == whole.out and np.array_equal(hashes, whole.hashes), (name, fresh)
            assert calls >= len(text) // fresh


def test_emit_limits_and_arguments(golden, tmp_path):
    lib = _lib.load()
    inp, nx, tso = case_files(golden["custom_indexes"], tmp_path)
    text = open(inp, "rb").read()
    sets = sets_of(nx, tso)
    whole = _lib.demux_emit_host(text, sets)
    assert whole.info["n_kept"] > 0
    exact = _lib.demux_emit_host(text, sets, cap=len(whole.out), max_records=whole.info["n_records"])
    assert exact.out == whole.out and exact.guards_intact
    for kw in ({"cap": len(whole.out) - 1}, {"max_records": whole.info["n_records"] - 1}):
        with pytest.raises(_lib.C3Error) as e:
            _lib.demux_emit_host(text, sets, **kw)
        assert e.value.code == _lib.E_LIMIT and e.value.untouched and e.value.guards_intact
        assert e.value.info["n_records"] == whole.info["n_records"]
    assert e.value.info["out_bytes"] == 0
    with pytest.raises(_lib.C3Error) as e:
        _lib.demux_emit_host(text, sets, cap=0)
    assert e.value.info["out_bytes"] == len(whole.out)
    assert _lib.demux_emit_host(b"", sets).info == {"n_records": 0, "n_kept": 0, "consumed": 0, "out_bytes": 0, "departed": 0}
    # the index limits and their texts are those of c3_demux_indexes
    one = _lib.DemuxSets(["A1"], ["ACGT"], ["B1", "B2"], ["AC", "GT"])
    long_ = _lib.DemuxSets(["A1", "A2"], ["ACGT" * 9, "AC"], ["B1", "B2"], ["AC", "GT"])
    for bad, code, msg in ((one, _lib.E_ARG, "at least 2 indexes"), (long_, _lib.E_LIMIT, "index longer than 32 bytes")):
        with pytest.raises(_lib.C3Error) as e:
            _lib.demux_emit_host(text, bad)
        assert e.value.code == code and msg in str(e.value)
    info = _lib.DemuxInfo()
    out = np.zeros(len(whole.out) + 8, dtype=np.uint8)
    hs = np.zeros(whole.info["n_records"] + 1, dtype=np.uint64)
    args = [text, len(text), 1] + list(sets.args) + [out.ctypes.data, out.size, hs.ctypes.data, hs.size, C.byref(info)]
    assert lib.c3_demux_emit_host(*args) == 0 and info.out_bytes == len(whole.out)
    for k in (0, 7, 12, 13, 15, 17):
        bad = list(args)
        bad[k] = None
        assert lib.c3_demux_emit_host(*bad) == _lib.E_ARG, k
        assert lib.c3_demux_emit(None, *bad) == _lib.E_ARG, k
    assert lib.c3_demux_emit(None, *args) == _lib.E_ARG
    assert lib.c3_demux_emit_timing(None, None) == _lib.E_ARG
