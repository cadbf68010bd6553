"""Strict four-line FASTQ (include/c3poa.h "FASTQ records on the GPU"): the host statement c3_fastq_parse_host against a small
parser of the rule written here (it shares nothing with the C++), on valid corpora, on every kind of departure at the first,
the second and the last record, on capacity and argument errors, and the command line's --parse gpu argument check.  The
corpora are the ones tests/test_gpu_fastq.py runs through k_fastq."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from c3poa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------
def ref_parse(text, at_eof=False, min_len=0):
    """the contract: (records [(name, seq, qual)], n_short, consumed, departed)"""
    whole = text if (at_eof and not text.endswith(b"\n")) else text[:text.rfind(b"\n") + 1]
    lines = whole.split(b"\n") if whole else []
    if whole.endswith(b"\n"):
        lines.pop()
    recs, n_short, consumed, departed = [], 0, 0, 0
    for i in range(0, len(lines), 4):
        if len(lines) - i < 4:
            departed = int(bool(at_eof))
            break
        h, s, p, q = [x[:-1] if x.endswith(b"\r") else x for x in lines[i:i + 4]]
        if not (h[:1] == b"@" and s and s[:1] not in (b"@", b">", b"+") and p[:1] == b"+" and len(q) == len(s)):
            departed = 1
            break
        consumed = min(len(text), consumed + sum(len(x) + 1 for x in lines[i:i + 4]))
        if len(s) < min_len:
            n_short += 1
        else:
            recs.append((re.split(rb"[ \t]", h[1:], maxsplit=1)[0], s, q))
    return recs, n_short, consumed, departed


def check(res, text, at_eof=False, min_len=0, what=""):
    """a FastqParse against the reference, field for field"""
    recs, n_short, consumed, departed = ref_parse(text, at_eof, min_len)
    want = {"n_records": len(recs) + n_short, "n_kept": len(recs), "n_short": n_short, "consumed": consumed,
            "name_bytes": sum(len(r[0]) for r in recs), "base_bytes": sum(len(r[1]) for r in recs), "departed": departed}
    assert res.info == want, what
    assert res.records() == recs, what
    assert res.names == b"".join(r[0] for r in recs) and res.seqs == b"".join(r[1] for r in recs), what
    assert res.quals == b"".join(r[2] for r in recs), what
    assert list(res.name_off) == list(np.cumsum([0] + [len(r[0]) for r in recs])), what
    assert list(res.off) == list(np.cumsum([0] + [len(r[1]) for r in recs])), what
    assert res.guards_intact and res.untouched_beyond_results, what


def same(a, b, what=""):
    """two FastqParse results, field for field"""
    assert a.info == b.info, what
    assert (a.names, a.seqs, a.quals) == (b.names, b.seqs, b.quals), what
    assert list(a.name_off) == list(b.name_off) and list(a.off) == list(b.off), what


# ---- corpora ------------------------------------------------------------------------------------------------------------
def rec(name, n, seed=0, eol=b"\n", qual0=None):
    rng = np.random.default_rng(1000 * n + seed)
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    qual = bytes(rng.integers(35, 74, n, dtype=np.uint8))            # '#' .. 'I' ('+' and '@' among them)
    if qual0 is not None and n:
        qual = qual0 + qual[1:]
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]
THREE = rec(b"first", 5) + rec(b"second some comment", 64) + rec(b"t", 3)


def valid_corpus():
    """(name, text, at_eof, min_len)"""
    out = []
    lens = b"".join(rec(b"r%d" % n, n) for n in LENGTHS)
    out.append(("lengths", lens, False, 0))
    out.append(("lengths at eof", lens, True, 0))
    names = (rec(b"a", 7) + rec(b"b c", 8) + rec(b"name\twith tab", 9) + rec(b"x  two blanks", 4) + rec(b"y\t", 5) + rec(b"", 6)
             + rec(b" leading", 3))
    out.append(("names", names, False, 0))
    out.append(("crlf", b"".join(rec(b"c%d desc" % n, n, eol=b"\r\n") for n in LENGTHS), False, 0))
    out.append(("crlf at eof, no last newline", b"".join(rec(b"c%d" % n, n, eol=b"\r\n") for n in (5, 64))[:-1], True, 0))
    out.append(("quality starts with @ and +", rec(b"q1", 6, qual0=b"@") + rec(b"q2", 65, qual0=b"+") + rec(b"q3", 1, qual0=b"@")
                + rec(b"q4", 1, qual0=b"+"), False, 0))
    out.append(("no last newline, at eof", THREE[:-1], True, 0))
    out.append(("no last newline, not at eof", THREE[:-1], False, 0))
    mixed = b"".join(rec(b"m%d" % i, n, seed=i) for i, n in enumerate([10, 3, 4, 300, 1, 5, 4, 2, 77]))
    for ml in (4, 5, 78, 1000):
        out.append(("min_len %d" % ml, mixed, False, ml))
    out.append(("empty", b"", False, 0))
    out.append(("empty at eof", b"", True, 0))
    out.append(("no newline at all", b"@abc", False, 0))
    return out


def cut_corpus():
    """THREE cut at every byte (not at_eof: the cut record is merely incomplete)"""
    return [("cut %d" % k, THREE[:k], False, 0) for k in range(len(THREE) + 1)]


DEPARTURES = [("blank line", b"\n"),
              ("fasta record", b">x\nACGT\n"),
              ("two-line sequence", b"@m\nACGT\nACGT\n+\nIIIIIIII\n"),
              ("quality one short", b"@q\nACGT\n+\nIII\n"),
              ("quality one long", b"@q\nACGT\n+\nIIIII\n"),
              ("line 2 not +", b"@p\nACGT\n-\nIIII\n"),
              ("sequence starts with +", b"@s\n+CGT\n+\nIIII\n"),
              ("empty sequence", b"@e\n\n+\n\n")]


def departure_corpus():
    """(name, text, at_eof, start of the departing record, strict records in front of it)"""
    good = [rec(b"g%d x" % i, n) for i, n in enumerate([6, 64, 5, 257])]
    out = []
    for kind, bad in DEPARTURES:
        for pos, where in ((0, "record 0"), (1, "record 1"), (len(good), "last record")):
            text = b"".join(good[:pos]) + bad + b"".join(good[pos:])
            start = sum(len(g) for g in good[:pos])
            # at the very end a departure shows only with at_eof: short of four lines it is otherwise an incomplete record
            for at_eof in ((True,) if pos == len(good) else (False, True)):
                out.append(("%s as %s%s" % (kind, where, ", at eof" if at_eof else ""), text, at_eof, start, pos))
    return out


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_valid_corpus():
    for name, text, at_eof, min_len in valid_corpus():
        check(_lib.fastq_parse_host(text, at_eof, min_len), text, at_eof, min_len, name)
    # the properties the corpus is there for, stated directly
    r = _lib.fastq_parse_host(THREE[:-1], True)
    assert r.info["n_records"] == 3 and r.info["consumed"] == len(THREE) - 1 and r.info["departed"] == 0
    r = _lib.fastq_parse_host(THREE[:-1], False)
    assert r.info["n_records"] == 2 and r.info["consumed"] == len(THREE) - len(rec(b"t", 3)) and r.info["departed"] == 0
    r = _lib.fastq_parse_host(valid_corpus()[2][1])
    assert [x[0] for x in r.records()] == [b"a", b"b", b"name", b"x", b"y", b"", b""]
    r = _lib.fastq_parse_host(b"".join(rec(b"c%d" % n, n, eol=b"\r\n") for n in LENGTHS))
    assert [len(x[1]) for x in r.records()] == LENGTHS and not any(b"\r" in x[1] + x[2] + x[0] for x in r.records())


def test_cut_at_every_byte():
    ends = np.cumsum([len(rec(b"first", 5)), len(rec(b"second some comment", 64)), len(rec(b"t", 3))])
    whole = _lib.fastq_parse_host(THREE).records()
    assert len(whole) == 3
    for name, text, at_eof, min_len in cut_corpus():
        r = _lib.fastq_parse_host(text, at_eof, min_len)
        check(r, text, at_eof, min_len, name)
        n_whole = int((ends <= len(text)).sum())
        assert r.info["consumed"] == (ends[n_whole - 1] if n_whole else 0) and r.info["departed"] == 0, name
        assert r.records() == whole[:n_whole], name
        check(_lib.fastq_parse_host(text, True, 0), text, True, 0, name + " at eof")


def test_text_at_every_offset_of_a_dword():
    for off in range(4):
        for name, text, at_eof, min_len in valid_corpus()[:3]:
            check(_lib.fastq_parse_host(text, at_eof, min_len, text_offset=off), text, at_eof, min_len, name)


def test_departures():
    cases = departure_corpus()
    assert len(cases) == len(DEPARTURES) * 5
    for name, text, at_eof, start, n_before in cases:
        r = _lib.fastq_parse_host(text, at_eof)
        assert r.info["departed"] == 1 and r.info["consumed"] == start and r.info["n_records"] == n_before, name
        check(r, text, at_eof, 0, name)
        check(_lib.fastq_parse_host(text[:start], at_eof), text[:start], at_eof, 0, name)       # the records in front: intact
        assert r.records() == _lib.fastq_parse_host(text[:start]).records(), name


def test_capacity_errors():
    text = b"".join(rec(b"n%d" % i, n) for i, n in enumerate([10, 20, 30]))
    need = _lib.fastq_parse_host(text).info
    assert (need["n_kept"], need["name_bytes"], need["base_bytes"]) == (3, 6, 60)
    check(_lib.fastq_parse_host(text, caps=(6, 60, 3)), text)                                   # exactly enough
    for caps in ((5, 60, 3), (6, 59, 3), (6, 60, 2), (0, 0, 0)):
        with pytest.raises(_lib.C3Error) as e:
            _lib.fastq_parse_host(text, caps=caps)
        assert e.value.code == _lib.E_LIMIT and e.value.info == need, caps
        assert e.value.guards_intact and e.value.untouched, caps                               # nothing half written
    with pytest.raises(_lib.C3Error) as e:                                                      # min_len counts: only kept records need room
        _lib.fastq_parse_host(text, min_len=20, caps=(3, 49, 2))
    assert e.value.code == _lib.E_LIMIT and e.value.info["n_kept"] == 2 and e.value.info["base_bytes"] == 50
    check(_lib.fastq_parse_host(text, min_len=20, caps=(4, 50, 2)), text, False, 20)


def _raw_args(text):
    n = len(text)
    names, seqs, quals = (C.create_string_buffer(n + 1) for _ in range(3))
    noff, off = ((C.c_int64 * (n + 2))() for _ in range(2))
    info = _lib.FastqInfo()
    return [text, n, 0, 0, names, n, noff, seqs, quals, n, off, n, C.byref(info)], info


def test_argument_errors():
    lib = _lib.load()
    text = rec(b"a", 4)
    args, info = _raw_args(text)
    assert lib.c3_fastq_parse_host(*args) == 0 and info.n_kept == 1
    for k in (0, 4, 6, 7, 8, 10, 12):                                   # every pointer
        bad = list(args)
        bad[k] = None
        assert lib.c3_fastq_parse_host(*bad) == _lib.E_ARG, k
    for k in (1, 5, 9, 11):                                             # every size
        bad = list(args)
        bad[k] = -1
        assert lib.c3_fastq_parse_host(*bad) == _lib.E_ARG, k
    assert b"bad arguments" in lib.c3_last_error(None)
    empty = list(args)
    empty[0], empty[1] = None, 0                                        # no text at all is fine
    assert lib.c3_fastq_parse_host(*empty) == 0 and info.n_records == 0 and info.consumed == 0
    # the device call refuses a null handle (and the same arguments) before it touches a GPU
    assert lib.c3_fastq_parse(None, *args) == _lib.E_ARG
    bad = list(args)
    bad[4] = None
    assert lib.c3_fastq_parse(None, *bad) == _lib.E_ARG
    # reader calls on no reader / on a reader that has no device inflater
    assert lib.c3_reader_parse_on_device(None, 1) == _lib.E_ARG
    assert lib.c3_reader_parse_stats(None, None, None, None) == _lib.E_ARG


def test_parse_device_needs_a_device_inflater(tmp_path):
    p = str(tmp_path / "a.fastq")
    open(p, "wb").write(THREE)
    with pytest.raises(_lib.C3Error) as e:
        _lib.Reader(p, parse_device=True)
    assert e.value.code == _lib.E_STATE
    rd = _lib.Reader(p)
    assert rd.parse_stats() == (0, 0, 0)
    assert rd.next(10).n == 3
    assert rd.lib.c3_reader_parse_on_device(rd.r, 1) == _lib.E_STATE
    rd.close()


def test_cli_parse_gpu_needs_inflate_gpu(tmp_path):
    fq = str(tmp_path / "r.fastq")
    open(fq, "wb").write(THREE)
    fa = str(tmp_path / "s.fasta")
    open(fa, "w").write(">S\nACGT\n")
    out = str(tmp_path / "out")
    for extra in (["--parse", "gpu"], ["--parse", "gpu", "--inflate", "host"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", fq, "-s", fa, "-o", out] + extra,
                           capture_output=True, text=True, env=dict(os.environ, C3_NO_EARLY_WARM="1"))
        assert p.returncode != 0, extra
        assert "--parse gpu needs --inflate gpu" in p.stderr, p.stderr
        assert not os.path.exists(out)                                  # refused in argument handling: nothing was started
    import C3POa
    assert C3POa.parse_args(["-r", fq, "-s", fa]).parse == "host"
    assert C3POa.parse_args(["-r", fq, "-s", fa, "--inflate", "gpu", "--parse", "gpu"]).parse == "gpu"
