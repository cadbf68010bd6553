"""CPU tests of c3_fastx_strict_parse_host (include/c3poa.h "Strict FASTA / FASTQ records"): on strict text of
both kinds it equals seqio.fastx_read; cut at any byte it consumes whole records only and the tail re-fed reproduces the
parse; every departure delivers exactly the records in front of it; too-small capacities report the need and write
nothing; and the flag combinations C3POa_postprocessing.py refuses are refused before anything is created."""
import os
import subprocess
import sys

import numpy as np
import pytest

from c3poa_amd import _lib
from c3poa_amd.seqio import fastx_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECS = [("read_1", "ACGTACGTAC", "IIIIIHHHHG"), ("r2", "G", "#"), ("third-read_9", "TTGACCA" * 9, "5" * 63)]


def text_of(recs, kind, eol=b"\n", comments=None, final_newline=True):
    out = b""
    for i, (name, seq, qual) in enumerate(recs):
        head = name.encode() + (comments[i] if comments else b"")
        if kind == 4:
            out += b"@" + head + eol + seq.encode() + eol + b"+" + eol + qual.encode() + eol
        else:
            out += b">" + head + eol + seq.encode() + eol
    return out if final_newline else out[:len(out) - len(eol)]


def fnv(name):
    h = 1469598103934665603
    for c in name:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def want(recs, kind):
    return [(n.encode(), s.encode(), q.encode() if kind == 4 else None) for n, s, q in recs]


def check_whole(text, recs, kind, at_eof=True):
    r = _lib.fastx_strict_parse_host(text, at_eof=at_eof, kind=kind)
    assert r.guards_intact and r.untouched_beyond_results
    assert r.info["departed"] == 0 and r.info["consumed"] == len(text) and r.info["n_records"] == len(recs)
    assert r.records() == want(recs, kind)
    assert list(r.hashes) == [fnv(n.encode()) for n, _s, _q in recs]
    return r


VARIANTS = [("plain", {}), ("crlf", {"eol": b"\r\n"}), ("no_final_newline", {"final_newline": False}),
            ("crlf_no_final_newline", {"eol": b"\r\n", "final_newline": False}),
            ("comments", {"comments": [b" a comment", b"\tafter a tab", b" two words\there"]})]


@pytest.mark.parametrize("kind", [2, 4])
@pytest.mark.parametrize("label,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_strict_text_equals_fastx_read(tmp_path, kind, label, kw):
    text = text_of(RECS, kind, **kw)
    p = tmp_path / ("in.fastq" if kind == 4 else "in.fasta")
    p.write_bytes(text)
    ref = [(n, s, q) for n, s, q in fastx_read(str(p))]
    assert ref == [(n, s, q if kind == 4 else None) for n, s, q in RECS]          # the reference reads what was written
    check_whole(text, RECS, kind)
    assert _lib.fastx_kind(text) == kind


@pytest.mark.parametrize("kind", [2, 4])
def test_one_base_record_and_empty_text(kind):
    check_whole(text_of([("x", "A", "!")], kind), [("x", "A", "!")], kind)
    for at_eof in (False, True):
        r = _lib.fastx_strict_parse_host(b"", at_eof=at_eof, kind=kind)
        assert r.info == {"n_records": 0, "consumed": 0, "name_bytes": 0, "base_bytes": 0, "departed": 0}
        assert list(r.off) == [0] and list(r.name_off) == [0]


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("kind", [2, 4])
def test_cut_at_every_byte_consumes_whole_records_and_the_tail_completes_the_parse(kind, eol):
    text = text_of(RECS, kind, eol=eol)
    bounds, at = [0], 0
    for k in range(len(RECS)):
        at += len(text_of(RECS[k:k + 1], kind, eol=eol))
        bounds.append(at)
    for cut in range(len(text) + 1):
        a = _lib.fastx_strict_parse_host(text[:cut], at_eof=False, kind=kind)
        assert a.info["departed"] == 0
        assert a.info["consumed"] == max(b for b in bounds if b <= cut), cut          # always a record boundary
        b = _lib.fastx_strict_parse_host(text[a.info["consumed"]:], at_eof=True, kind=kind)
        assert b.info["departed"] == 0 and b.info["consumed"] == len(text) - a.info["consumed"]
        assert a.records() + b.records() == want(RECS, kind), cut
        assert list(a.hashes) + list(b.hashes) == [fnv(n.encode()) for n, _s, _q in RECS]


def departures(kind):
    """(label, text, at_eof, records delivered): the departure sits behind `delivered` good records"""
    good = text_of(RECS[:2], kind)
    other = text_of(RECS[2:], 2 if kind == 4 else 4)
    last = text_of(RECS[2:], kind)
    out = [("blank_line", good + b"\n" + last, True, 2),
           ("blank_line_crlf", good + b"\r\n" + last, True, 2),
           ("other_kind", good + other, True, 2),
           ("other_kind_first", other + good, True, 0),
           ("neither_kind_first", b"ACGT\n" + good, True, 0),
           ("incomplete_at_eof", good + last[:last.index(b"\n") + 1], True, 2),
           ("header_only_at_eof_no_newline", good + last[:5], True, 2),
           ("high_byte_in_name", good + last[:3] + b"\xc3\xa9" + last[3:], True, 2),
           ("high_byte_in_sequence", good + last[:last.index(b"\n") + 3] + b"\x80" + last[last.index(b"\n") + 3:], True, 2),
           ("high_byte_in_first_record", b">\xff"[:2] + good, True, 0)]
    n, s, q = RECS[2]
    if kind == 2:
        out += [("empty_sequence_line", good + b">" + n.encode() + b"\n\n", True, 2),
                # the second sequence line stands where a header is due: the departure lies behind the record's first two lines
                ("multi_line_sequence", good + b">" + n.encode() + b"\n" + s[:20].encode() + b"\n" + s[20:].encode() + b"\n" + good, True, 3)]
    else:
        out += [("empty_sequence_line", good + b"@" + n.encode() + b"\n\n+\n\n", True, 2),
                ("multi_line_sequence", good + b"@" + n.encode() + b"\n" + s[:20].encode() + b"\n" + s[20:].encode() + b"\n+\n" + q.encode() + b"\n", True, 2),
                ("unequal_lengths", good + b"@" + n.encode() + b"\n" + s.encode() + b"\n+\n" + q[:-1].encode() + b"\n", True, 2),
                ("high_byte_in_quality", good + b"@" + n.encode() + b"\n" + s.encode() + b"\n+\n" + b"\x90" + q[1:].encode() + b"\n", True, 2)]
    return out


@pytest.mark.parametrize("kind", [2, 4])
def test_every_departure_delivers_exactly_the_records_in_front_of_it(kind):
    seen = set()
    for label, text, at_eof, delivered in departures(kind):
        r = _lib.fastx_strict_parse_host(text, at_eof=at_eof, kind=kind)
        assert r.guards_intact and r.untouched_beyond_results, label
        assert r.info["departed"] == 1, label
        assert r.info["n_records"] == delivered, label
        got = r.records()
        if label == "multi_line_sequence" and kind == 2:
            assert got[:2] == want(RECS[:2], kind) and got[2] == (RECS[2][0].encode(), RECS[2][1][:20].encode(), None)
        else:
            assert got == want(RECS[:delivered], kind), label
        assert text[:r.info["consumed"]] == b"".join(text_of([(n.decode(), s.decode(), (q or b"").decode())], kind) for n, s, q in got), label
        seen.add(label)
    assert {"blank_line", "multi_line_sequence", "empty_sequence_line", "other_kind", "high_byte_in_name", "incomplete_at_eof"} <= seen


@pytest.mark.parametrize("kind", [2, 4])
def test_incomplete_record_without_at_eof_is_no_departure(kind):
    text = text_of(RECS, kind)
    r = _lib.fastx_strict_parse_host(text[:-3], at_eof=False, kind=kind)
    assert r.info["departed"] == 0 and r.info["n_records"] == 2
    r = _lib.fastx_strict_parse_host(text[:-3], at_eof=True, kind=kind)            # ... with it, the cut sequence line is the last line
    assert (r.info["departed"], r.info["n_records"]) == ((0, 3) if kind == 2 else (1, 2))


@pytest.mark.parametrize("kind", [2, 4])
def test_limit_reports_the_need_and_writes_nothing(kind):
    text = text_of(RECS, kind)
    full = _lib.fastx_strict_parse_host(text, at_eof=True, kind=kind).info
    nb, sb, nr = full["name_bytes"], full["base_bytes"], full["n_records"]
    assert (nb, sb, nr) == (sum(len(r[0]) for r in RECS), sum(len(r[1]) for r in RECS), 3)
    for caps in [(nb - 1, sb, nr), (nb, sb - 1, nr), (nb, sb, nr - 1), (0, 0, 0)]:
        with pytest.raises(_lib.C3Error) as e:
            _lib.fastx_strict_parse_host(text, at_eof=True, kind=kind, caps=caps)
        assert e.value.code == _lib.E_LIMIT
        assert e.value.info == full and e.value.guards_intact and e.value.untouched
    r = _lib.fastx_strict_parse_host(text, at_eof=True, kind=kind, caps=(nb, sb, nr))    # exactly enough
    assert r.records() == want(RECS, kind) and r.guards_intact


def test_null_arguments_and_bad_kinds_are_refused():
    import ctypes as C
    lib = _lib.load()
    text = text_of(RECS, 4)
    bufs = [np.zeros(256, dtype=np.uint8) for _ in range(6)]
    names, name_off, seqs, quals, off, hashes = [b.ctypes.data for b in bufs]
    info = _lib.FastxInfo()

    def call(**kw):
        a = dict(text=text, n=len(text), kind=4, names=names, name_off=name_off, seqs=seqs, quals=quals, off=off, hashes=hashes,
                 info=C.byref(info), names_cap=64, bases_cap=128, max_records=8)
        a.update(kw)
        return lib.c3_fastx_strict_parse_host(a["text"], a["n"], 1, a["kind"], a["names"], a["names_cap"], a["name_off"], a["seqs"], a["quals"],
                                              a["bases_cap"], a["off"], a["hashes"], a["max_records"], a["info"])

    assert call() == 0 and info.n_records == 3
    for kw in [{"text": None}, {"names": None}, {"name_off": None}, {"seqs": None}, {"quals": None}, {"off": None}, {"hashes": None},
               {"info": None}, {"n": -1}, {"names_cap": -1}, {"bases_cap": -1}, {"max_records": -1}, {"kind": 0}, {"kind": 3}, {"kind": 8}]:
        assert call(**kw) == _lib.E_ARG, kw
        assert b"c3_fastx_strict_parse_host" in lib.c3_last_error(None)
    assert call(text=text_of(RECS, 2), n=len(text_of(RECS, 2)), kind=2, quals=None) == 0          # kind 2 needs no quals
    assert call(text=None, n=0) == 0 and info.n_records == 0                                      # text may be null when n == 0
    assert call(n=_lib.FASTA_MAX_TEXT + 1) == _lib.E_LIMIT


REFUSED = [(["--bgzf"], "--bgzf needs --emit gpu"),
           (["--parse", "gpu"], "--parse gpu needs --emit gpu"),
           (["--emit", "gpu", "--inflate", "gpu"], "--inflate gpu needs --parse gpu"),
           (["--emit", "gpu", "--bgzf", "-co"], "-co and --bgzf")]


@pytest.mark.parametrize("flags,message", REFUSED, ids=[" ".join(f) for f, _m in REFUSED])
def test_cli_refuses_flag_combinations_before_anything_is_created(tmp_path, flags, message):
    out = tmp_path / "out"
    fa = tmp_path / "in.fasta"
    fa.write_bytes(text_of(RECS, 2))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "C3POa_postprocessing.py"), "-i", str(fa), "-a", str(fa), "-o", str(out)] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 2 and message in r.stderr, r.stderr
    assert not out.exists()
